// The roots of many independent commitment lists in one call (DESIGN.md "Roots of many lists"): list i is leaves[first .. first + count) of one shared array, and
// its root is notes.cpp's merkle_root over that list alone at depth d, 1 <= d <= 32 — the tree of gpu_tree.hip, one small tree per list instead of one resident
// tree: a node is one compression of left || right from the standard IV, a missing right child at level k is empty[k], an empty list has root empty[d].
// One kernel, launched once per size class of the call: a class holds the lists of 2^lgL < count <= 2^(lgL + 1) nodes (lgL = 0: up to two), a workgroup serves
// 256 >> lgL of them with 2^lgL lanes each.  A list of more than LIST_TILE nodes is first cut into aligned tiles of LIST_TILE nodes, each tile a list of the widest
// class whose "root" — its one node nine levels up — goes to a scratch array; that repeats until the list is down to LIST_TILE nodes and joins the classes with the
// level reached as its base level.  The number of launches of a call follows from the classes and passes it has, never from the number of lists or of levels.
// Everything runs in order on the library's main stream (lane 0); the caller holds the device mutex.
#include <algorithm>
#include <atomic>
#include <cstring>
#include "gpu_internal.hpp"
#include "tree_sha256.cuh"

namespace zk {
void sha256_compress_raw(const uint8_t left[32], const uint8_t right[32], uint8_t out[32]);   // notes.cpp (the empty roots)

constexpr int LIST_THREADS = 256, LIST_TILE_LOG = 9, LIST_TILE = 1 << LIST_TILE_LOG;   // a workgroup's lanes; the widest list a workgroup takes: two nodes a lane
constexpr uint32_t LIST_IN_HASH = 1, LIST_OUT_HASH = 2;

// one list of a launch: `count` nodes from node `first` of the launch's source array, the result to node `out` of its destination (count <= 2 << lgL)
struct RootJob { uint64_t first; uint32_t count, out; };

// hash order: message word i of a node is the plain little-endian word 7 - i of its 32 bytes, so this order needs no byte swap, only the reversed index
__device__ __forceinline__ Node list_load(const uint8_t *p, bool hash) {
  if (!hash) return tree_load(p);
  const uint4 a = ((const uint4 *)p)[0], b = ((const uint4 *)p)[1]; return {{b.w, b.z, b.y, b.x, a.w, a.z, a.y, a.x}};
}
__device__ __forceinline__ void list_store(uint8_t *p, const Node &v, bool hash) {
  if (!hash) { tree_store(p, v); return; }
  ((uint4 *)p)[0] = make_uint4(v.w[7], v.w[6], v.w[5], v.w[4]); ((uint4 *)p)[1] = make_uint4(v.w[3], v.w[2], v.w[1], v.w[0]);
}

// A group of L = 2^lgL lanes owns one list whose nodes lie at level k0 and carries it lgL + 1 levels up, one lane one node, the nodes of the level just made lying
// in LDS (as words) for the next one: level k0 + j has at most L >> (j - 1) nodes a list, so the groups' shares of a level are packed side by side — 256 nodes
// after the first level, 128 after the second, ping-pong — and every list of the launch takes the same number of barriers.  A list shorter than its class allows
// is down to one node early; lane 0 of its group then simply goes on pairing it with empty[k].  After the last LDS level each list is one node, written by its
// group's lane 0 — a lane makes node t of every level, lane 0 always node 0 —: the other lanes leave, lane 0 takes its node back (through LDS and not a register
// carried round the loop: eight registers the compression needs) and walks compress(node, empty[k]) up to `depth` without barriers.  A tile pass is the same kernel with lgL = 8 and depth = k0 + 9: no chain, the node goes to the scratch array in blob order.
__global__ void __launch_bounds__(LIST_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) k_list_roots(const uint8_t *src,
    const RootJob *__restrict__ jobs, uint32_t n_jobs, uint32_t lgL, uint32_t k0, uint32_t depth, const uint8_t *__restrict__ empty, uint8_t *dst, uint32_t flags) {
  __shared__ uint4 lds_a[LIST_THREADS * 2], lds_b[LIST_THREADS];
  const uint32_t tid = threadIdx.x, g = tid >> lgL, t = tid & ((1u << lgL) - 1), levels = lgL + 1;
  const uint64_t job = (uint64_t)blockIdx.x * (LIST_THREADS >> lgL) + g; const bool live = job < n_jobs;
  // (the job is read where it is needed and not kept: its words would live in registers beside the sixteen of the message schedule)
  uint32_t p_cnt = live ? jobs[job].count : 0;
#pragma unroll 1
  for (uint32_t j = 1; j <= levels; j++) {
    const uint32_t cnt = (p_cnt + 1) >> 1, width = (1u << lgL) >> (j - 1);                      // nodes of this level; a group's share of the level's LDS array
    const uint4 *from = (j & 1) ? lds_b : lds_a; uint4 *to = (j & 1) ? lds_a : lds_b;           // level k0 + 1 goes to lds_a
    if (t < cnt) {
      const uint32_t c = 2 * t; const bool lone = c + 1 >= p_cnt; Node l, r;
      if (j == 1) {
        const uint8_t *below = src + 32 * (jobs[job].first + c); const bool in_hash = flags & LIST_IN_HASH;
        l = list_load(below, in_hash); if (!lone) r = list_load(below + 32, in_hash);
      } else {
        const uint4 *q = from + 2 * (g * 2 * width + c); l = {{q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w}};
        if (!lone) r = {{q[2].x, q[2].y, q[2].z, q[2].w, q[3].x, q[3].y, q[3].z, q[3].w}};
      }
      if (lone) r = tree_load(empty + 32 * (k0 + j - 1));
      const Node v = tree_compress(l, r);
      to[2 * (g * width + t)] = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]); to[2 * (g * width + t) + 1] = make_uint4(v.w[4], v.w[5], v.w[6], v.w[7]);
    }
    if (j < levels) __syncthreads();
    p_cnt = cnt;
  }
  if (t || !live) return;
  const RootJob J = jobs[job]; Node v;
  if (!J.count) v = tree_load(empty + 32 * depth);                                              // (an empty list: no node was made; only with k0 = 0)
  else {
    const uint4 *top = ((levels & 1) ? lds_a : lds_b) + 2 * g; v = {{top[0].x, top[0].y, top[0].z, top[0].w, top[1].x, top[1].y, top[1].z, top[1].w}};   // (this lane's own write)
#pragma unroll 1
    for (uint32_t k = k0 + levels; k < depth; k++) v = tree_compress(v, tree_load(empty + 32 * k));
  }
  list_store(dst + 32 * (uint64_t)J.out, v, flags & LIST_OUT_HASH);
}

namespace {
std::atomic<uint64_t> g_list_root_launches{0};
template <class T> void grow(DevBuf<T> &b, size_t n) { if (n > b.size()) b = DevBuf<T>(n + n / 4 + 64); }
struct Workspace {
  DevBuf<uint8_t> leaves, scratch, roots, empty, jobs /* RootJob */; std::vector<RootJob> host_jobs;
  Workspace() : empty(32 * 33) {                                                                // empty[k] for every depth: it does not depend on the tree's
    uint8_t e[32 * 33] = {0}; for (int k = 1; k <= 32; k++) sha256_compress_raw(e + 32 * (k - 1), e + 32 * (k - 1), e + 32 * k);
    empty.upload(e, sizeof e);
  }
};
Workspace &workspace() { static Workspace *w = new Workspace(); return *w; }                    // one a process; the caller holds the device mutex
struct Launch { bool from_scratch, to_scratch; size_t job0, n_jobs; uint32_t lgL, k0, depth, flags; };
uint32_t class_of(uint64_t count) { uint32_t lg = 0; while ((2ull << lg) < count) lg++; return lg; }   // count <= LIST_TILE: the smallest lgL with count <= 2 << lgL
}  // namespace

uint64_t list_roots_launches() { return g_list_root_launches.load(); }

void list_roots_dev(int depth, const uint8_t *leaves, size_t n_leaves, const LeafRange *lists, size_t n_lists, bool hash_order, uint8_t *roots) {
  if (depth < 1 || depth > 32) throw GpuError("list roots: the depth must lie between 1 and 32");
  if (!n_lists) return;
  if (n_lists >= (1ull << 32)) throw GpuError("list roots: more than 2^32 - 1 lists in one call");
  LaneScope lane(0); Workspace &W = workspace(); hipStream_t s = gpu().stream;
  // The plan: every launch's jobs in one array.  First the lists of at most LIST_TILE leaves by class, straight from the leaves to the roots; then the passes over
  // the longer ones; then those lists again by (base level, class), from the scratch array to the roots.
  std::vector<RootJob> &jobs = W.host_jobs; jobs.clear(); std::vector<Launch> plan; size_t scratch_nodes = 0;
  { HostSpan span("host.roots_plan");
    const uint32_t io = hash_order ? LIST_IN_HASH | LIST_OUT_HASH : 0;
    struct Long { uint64_t first, count; uint32_t out; }; std::vector<Long> cur, next, done[4];   // done[p]: down to LIST_TILE nodes after pass p - 1, at level 9 p
    size_t per_class[LIST_TILE_LOG] = {0};
    for (size_t i = 0; i < n_lists; i++) {
      if (lists[i].count > (1ull << depth) || lists[i].first > n_leaves || lists[i].count > n_leaves - lists[i].first) throw GpuError("list roots: a range the caller did not check");
      if (lists[i].count <= LIST_TILE) per_class[class_of(lists[i].count)]++; else cur.push_back({lists[i].first, lists[i].count, (uint32_t)i});
    }
    size_t at[LIST_TILE_LOG], total = 0;
    for (int c = 0; c < LIST_TILE_LOG; c++) { at[c] = total; if (per_class[c]) plan.push_back({false, false, total, per_class[c], (uint32_t)c, 0, (uint32_t)depth, io}); total += per_class[c]; }
    jobs.resize(total);
    for (size_t i = 0; i < n_lists; i++) if (lists[i].count <= LIST_TILE) jobs[at[class_of(lists[i].count)]++] = {lists[i].first, (uint32_t)lists[i].count, (uint32_t)i};
    for (uint32_t p = 0; !cur.empty(); p++) {                                                   // (count <= 2^32: at most three passes)
      const size_t job0 = jobs.size(); next.clear();
      for (const Long &l : cur) {
        const uint64_t tiles = (l.count + LIST_TILE - 1) >> LIST_TILE_LOG;
        if (scratch_nodes + tiles >= (1ull << 32)) throw GpuError("list roots: the long lists of one call need more than 2^32 scratch nodes");
        for (uint64_t k = 0; k < tiles; k++) jobs.push_back({l.first + (k << LIST_TILE_LOG), (uint32_t)std::min<uint64_t>(LIST_TILE, l.count - (k << LIST_TILE_LOG)), (uint32_t)(scratch_nodes + k)});
        (tiles <= LIST_TILE ? done[p + 1] : next).push_back({scratch_nodes, tiles, l.out}); scratch_nodes += tiles;
      }
      plan.push_back({p > 0, true, job0, jobs.size() - job0, (uint32_t)LIST_TILE_LOG - 1, LIST_TILE_LOG * p, LIST_TILE_LOG * (p + 1), p ? 0u : (hash_order ? LIST_IN_HASH : 0u)});
      cur.swap(next);
    }
    for (uint32_t p = 1; p < 4; p++) {
      std::stable_sort(done[p].begin(), done[p].end(), [](const Long &a, const Long &b) { return class_of(a.count) < class_of(b.count); });
      for (size_t i = 0; i < done[p].size();) {
        const uint32_t c = class_of(done[p][i].count); const size_t job0 = jobs.size();
        for (; i < done[p].size() && class_of(done[p][i].count) == c; i++) jobs.push_back({done[p][i].first, (uint32_t)done[p][i].count, done[p][i].out});
        plan.push_back({true, false, job0, jobs.size() - job0, c, LIST_TILE_LOG * p, (uint32_t)depth, hash_order ? LIST_OUT_HASH : 0u});
      }
    }
  }
  grow(W.leaves, 32 * n_leaves); grow(W.roots, 32 * n_lists); grow(W.scratch, 32 * scratch_nodes); grow(W.jobs, jobs.size() * sizeof(RootJob));
  bool queued = false;
  try {
    { Stage up("roots.upload"); queued = true;
      if (n_leaves) HIP_CHECK(hipMemcpyAsync(W.leaves.get(), leaves, 32 * n_leaves, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(W.jobs.get(), jobs.data(), jobs.size() * sizeof(RootJob), hipMemcpyHostToDevice, s)); }
    { Stage st("roots.kernels");
      for (const Launch &L : plan) {
        const size_t per_group = LIST_THREADS >> L.lgL, blocks = (L.n_jobs + per_group - 1) / per_group;
        if (L.n_jobs >= (1ull << 32) || blocks >= (1ull << 31)) throw GpuError("list roots: a launch of more than 2^31 workgroups");
        hipLaunchKernelGGL(k_list_roots, dim3((unsigned)blocks), dim3(LIST_THREADS), 0, s, L.from_scratch ? W.scratch.get() : W.leaves.get(), (const RootJob *)W.jobs.get() + L.job0,
            (uint32_t)L.n_jobs, L.lgL, L.k0, L.depth, W.empty.get(), L.to_scratch ? W.scratch.get() : W.roots.get(), L.flags);
        g_list_root_launches.fetch_add(1);
      }
      HIP_CHECK(hipGetLastError()); }
    { Stage dn("roots.download"); HIP_CHECK(hipMemcpyAsync(roots, W.roots.get(), 32 * n_lists, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s)); }
  } catch (...) { if (queued) (void)hipStreamSynchronize(s); throw; }   // (no copy may still read the caller's memory or the plan once the call has returned)
}

}  // namespace zk
