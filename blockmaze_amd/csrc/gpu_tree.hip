// The commitment tree resident in HBM (DESIGN.md "Commitment tree"): an append-only SHA-256 Merkle tree of depth d, 1 <= d <= 32, as notes.cpp:tree_levels
// restates it from IncrementalMerkleTree.tcc:179-258 — node = one compression of left || right from the standard IV, no padding; leaves are 32-byte blobs in blob
// byte order; an unseen leaf is all zero, so a missing right sibling at level k is the empty root empty[k].
// Layout: level k (0 = leaves ... d = root) holds c_k = ceil(n / 2^k) nodes, at least one once a leaf exists — above the first level with a single node that is the
// spine of compress(node, empty[k]).  All levels lie in one allocation: with a leaf capacity cap0 = 2^c level k has room for max(cap0 >> k, 1) nodes and starts at
// node offset tree_off(k).  Nodes are stored as bytes, so a path is a gather and a download.
// Everything runs in order on the library's main stream (lane 0) under the device mutex, each entry of a tree under that tree's own mutex.
#include <cstring>
#include <mutex>
#include "gpu_internal.hpp"
#include "tree_sha256.cuh"

extern std::mutex g_gpu_mutex;

namespace zk {
void sha256_compress_raw(const uint8_t left[32], const uint8_t right[32], uint8_t out[32]);   // notes.cpp (the empty roots, 32 compressions a tree)

constexpr int TREE_TILE_LOG = 9, TREE_TILE = 1 << TREE_TILE_LOG;   // nodes of the base level a workgroup takes; it carries them TREE_TILE_LOG levels up
constexpr int TREE_THREADS = 256;
constexpr uint32_t TREE_MIN_CAP_LOG = 10;

struct TreeGeom { uint8_t *nodes; const uint8_t *empty; uint32_t cap_log, depth; };
__host__ __device__ __forceinline__ uint64_t tree_off(uint32_t cap_log, uint32_t k) {
  const uint64_t two = 2ull << cap_log; return k <= cap_log ? two - (two >> k) : two - 2 + (k - cap_log);
}
__device__ __forceinline__ uint64_t tree_count(uint64_t n, uint32_t k) { return (n >> k) + ((n & ((1ull << k) - 1)) ? 1 : 0); }   // ceil(n / 2^k), k <= 32

// The append kernel.  The tree grew from n_old to n_new leaves and levels 0 .. k0 are up to date; level k's dirty range is lo_k = floor(n_old / 2^k) ..
// c_k - 1 = ceil(n_new / 2^k) - 1, and nothing else of a level is computed.  A workgroup owns a window of level k0 and carries it `levels` levels up, the nodes of
// the level just made lying in LDS (as words) for the next one, one barrier a level:
//   tiled  (ragged = 0): the window is the aligned tile blockIdx.x + tile0 of TREE_TILE nodes, levels = TREE_TILE_LOG, so the tile ends in one node;
//   ragged (ragged = 1): one workgroup, the window is the whole dirty range of level k0 (at most TREE_TILE nodes), levels = depth - k0: once a level's dirty range
//                        is down to one node — the spine, or the single parent chain of a small append — lane 0 of the first wave walks it to the root alone, without barriers.
// Outside its LDS window a node's left child is clean (older than this append: read from the level's array) and its right child does not exist (empty[k]).
__global__ void __launch_bounds__(TREE_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) k_tree_append(TreeGeom G, uint64_t n_old, uint64_t n_new, uint32_t k0, uint32_t levels, uint64_t tile0, int ragged) {
  __shared__ uint4 lds_a[(TREE_TILE / 2 + 1) * 2], lds_b[(TREE_TILE / 4 + 2) * 2];
  const uint32_t tid = threadIdx.x;
  const uint64_t t_lo = ragged ? 0 : (tile0 + blockIdx.x) << TREE_TILE_LOG;                      // window at level k0 (ragged: bounded by the dirty range alone)
  // p_lo, p_cnt: this workgroup's nodes of the level below the one being made (all uniform: scalar registers)
  uint64_t p_lo = n_old >> k0; if (t_lo > p_lo) p_lo = t_lo;
  uint64_t p_hi = tree_count(n_new, k0); if (!ragged && t_lo + TREE_TILE < p_hi) p_hi = t_lo + TREE_TILE;
  uint32_t p_cnt = (uint32_t)(p_hi - p_lo); bool chain = false;
#pragma unroll 1
  for (uint32_t j = 1; j <= levels; j++) {
    const uint32_t k = k0 + j;
    uint64_t lo = n_old >> k; if ((t_lo >> j) > lo) lo = t_lo >> j;
    uint64_t hi = tree_count(n_new, k); if (!ragged && ((t_lo + TREE_TILE) >> j) < hi) hi = (t_lo + TREE_TILE) >> j;
    const uint32_t cnt = (uint32_t)(hi - lo); const int dl = (int)(2 * lo - p_lo);                 // 0, or -1: the first node's left child is clean
    if (ragged && p_cnt == 1 && !chain) { chain = true; if (tid) return; }                         // one dirty node below: lane 0 walks the rest, no barrier needed
    const uint8_t *below = G.nodes + 32 * (tree_off(G.cap_log, k - 1) + p_lo), *none = G.empty + 32 * (k - 1);
    uint8_t *here = G.nodes + 32 * (tree_off(G.cap_log, k) + lo);
    const uint4 *src = (j & 1) ? lds_b : lds_a; uint4 *dst = (j & 1) ? lds_a : lds_b;             // level k0 + 1 goes to lds_a (up to TREE_TILE / 2 + 1 nodes)
    for (uint32_t t = tid; t < cnt; t += TREE_THREADS) {
      const int c = 2 * (int)t + dl; Node l, r;
      if (j > 1 && c >= 0) { const uint4 x = src[2 * c], y = src[2 * c + 1]; l = {{x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w}}; }
      else l = tree_load(below + 32 * c);
      if ((uint32_t)(c + 1) >= p_cnt) r = tree_load(none);
      else if (j > 1) { const uint4 x = src[2 * c + 2], y = src[2 * c + 3]; r = {{x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w}}; }
      else r = tree_load(below + 32 * (c + 1));
      const Node v = tree_compress(l, r);
      tree_store(here + 32 * t, v);
      dst[2 * t] = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]); dst[2 * t + 1] = make_uint4(v.w[4], v.w[5], v.w[6], v.w[7]);
    }
    if (!chain) __syncthreads();
    p_lo = lo; p_cnt = cnt;
  }
}

// first index whose leaf equals the blob, 2^64 - 1 if none of the n leaves does
__global__ void __launch_bounds__(256) k_tree_find(const uint4 *__restrict__ leaves, uint64_t n, uint4 t0, uint4 t1, unsigned long long *__restrict__ first) {
  unsigned long long best = ~0ull;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 a = leaves[2 * i], b = leaves[2 * i + 1];
    if (a.x == t0.x && a.y == t0.y && a.z == t0.z && a.w == t0.w && b.x == t1.x && b.y == t1.y && b.z == t1.z && b.w == t1.w) { best = i; break; }   // (a lane's indices ascend)
  }
  if (best != ~0ull) atomicMin(first, best);
}
// out = [index: 8 bytes, padded to 32 | depth siblings of that leaf, leaf level first | root]; the index comes from the host or (index_dev) from k_tree_find's
// word.  An index that is no leaf (the blob was not found) leaves the siblings unwritten.
__global__ void __launch_bounds__(64) k_tree_path(TreeGeom G, uint64_t n, uint64_t index, const unsigned long long *__restrict__ index_dev, uint8_t *__restrict__ out) {
  const uint32_t k = threadIdx.x; if (index_dev) index = *index_dev;
  if (k == 0) { ((unsigned long long *)out)[0] = index; }
  if (k == G.depth) { const uint8_t *src = n ? G.nodes + 32 * tree_off(G.cap_log, G.depth) : G.empty + 32 * G.depth; ((uint4 *)(out + 32 * (G.depth + 1)))[0] = ((const uint4 *)src)[0]; ((uint4 *)(out + 32 * (G.depth + 1)))[1] = ((const uint4 *)src)[1]; }
  if (k >= G.depth || index >= n) return;
  const uint64_t sib = (index >> k) ^ 1; const uint8_t *src = sib < tree_count(n, k) ? G.nodes + 32 * (tree_off(G.cap_log, k) + sib) : G.empty + 32 * k;
  ((uint4 *)(out + 32 * (k + 1)))[0] = ((const uint4 *)src)[0]; ((uint4 *)(out + 32 * (k + 1)))[1] = ((const uint4 *)src)[1];
}

// ---- past states (DESIGN.md "Past states of the commitment tree") ---------------------------------------------------------------------------------------------
// State m, 1 <= m <= n, is the tree of the first m leaves.  It differs from the stored nodes only along its right edge, one node a level: B_k = node (m - 1) >> k of
// level k.  Where 2^k divides m that node is complete and stored, so the walk starts at k0 = min(ctz(m), depth) with the stored node; above it
//   B_k = compress(stored[k-1][j - 1], B_{k-1})  if j = (m - 1) >> (k - 1) is odd (the left sibling is a complete subtree: stored, and the same in every later state)
//       = compress(B_{k-1}, empty[k-1])           otherwise.
// One load a level — the sibling or the empty root, fetched before the compression of the level below runs — then the operands are selected and tree_compress is
// called ONCE: a wave whose lanes differ in parity runs one compression a level, and a kernel holds one copy of it.  sink(k, B_k) sees every level from k0 to depth.
__device__ __forceinline__ const uint8_t *tree_edge_operand(const TreeGeom &G, uint64_t m, uint32_t k) {   // the other operand of B_k's compression
  const uint64_t j = (m - 1) >> (k - 1);
  return (j & 1) ? G.nodes + 32 * (tree_off(G.cap_log, k - 1) + j - 1) : G.empty + 32 * (k - 1);
}
// Where m is the same for the whole launch (k_tree_paths_at, k_tree_rewind) the compiler would run the walk on the scalar ALU, which has no rotate: measured 7.5 us a
// level against 4 on the vector ALU.  The empty statement below holds the node in vector registers, and the compression follows it there.
__device__ __forceinline__ void tree_in_vgprs(Node &v) {
#pragma unroll
  for (int i = 0; i < 8; i++) asm volatile("" : "+v"(v.w[i]));
}
template <class Sink> __device__ __forceinline__ Node tree_edge_walk(const TreeGeom &G, uint64_t m, Sink sink) {
  const uint32_t tz = (uint32_t)__builtin_ctzll(m), k0 = tz < G.depth ? tz : G.depth;
  Node B = tree_load(G.nodes + 32 * (tree_off(G.cap_log, k0) + ((m - 1) >> k0))); tree_in_vgprs(B); sink(k0, B);
  if (k0 == G.depth) return B;
  Node o = tree_load(tree_edge_operand(G, m, k0 + 1));
#pragma unroll 1
  for (uint32_t k = k0 + 1; k <= G.depth; k++) {
    const bool odd = ((m - 1) >> (k - 1)) & 1; Node l, r;
#pragma unroll
    for (int i = 0; i < 8; i++) { l.w[i] = odd ? o.w[i] : B.w[i]; r.w[i] = odd ? B.w[i] : o.w[i]; }
    if (k < G.depth) o = tree_load(tree_edge_operand(G, m, k + 1));
    B = tree_compress(l, r); sink(k, B);
  }
  return B;
}
__device__ __forceinline__ void tree_copy32(uint8_t *dst, const uint8_t *src) { ((uint4 *)dst)[0] = ((const uint4 *)src)[0]; ((uint4 *)dst)[1] = ((const uint4 *)src)[1]; }

// out[t] = the root of state sizes[t], one lane a size; size 0 is the empty tree.  The host has checked sizes[t] <= n.
__global__ void __launch_bounds__(64) k_tree_roots_at(TreeGeom G, const unsigned long long *__restrict__ sizes, uint64_t q, uint8_t *__restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; if (t >= q) return;
  const uint64_t m = sizes[t];
  if (!m) { tree_copy32(out + 32 * t, G.empty + 32 * G.depth); return; }
  tree_store(out + 32 * t, tree_edge_walk(G, m, [](uint32_t, const Node &) {}));
}
// q leaves of ONE state m >= 1: out = [root of state m | index: 8 bytes, padded to 32 | q x depth siblings, leaf level first].  The indices come from the host
// (checked: below m) or, for q = 1, from k_tree_find's word (index_dev), which is then written to the index slot; an index that is no leaf of state m leaves the
// siblings unwritten.  Lane 0 of every workgroup walks the edge into LDS in blob byte order; after the barrier one lane per (leaf, level) gathers: the sibling
// s = (i >> k) ^ 1 is stored if its subtree is complete in state m, empty if it starts at or beyond m, and otherwise it is the edge node B_k.
__global__ void __launch_bounds__(256) k_tree_paths_at(TreeGeom G, uint64_t m, const unsigned long long *__restrict__ indices, const unsigned long long *__restrict__ index_dev,
                                                        uint64_t q, uint8_t *__restrict__ out) {
  __shared__ uint4 edge[2 * 33];
  if (threadIdx.x == 0) tree_edge_walk(G, m, [&](uint32_t k, const Node &B) { tree_store((uint8_t *)&edge[2 * k], B); });
  __syncthreads();
  const uint8_t *edge_bytes = (const uint8_t *)edge;
  if (blockIdx.x == 0 && threadIdx.x == 0) { tree_copy32(out, edge_bytes + 32 * G.depth); if (index_dev) ((unsigned long long *)out)[4] = *index_dev; }
  const uint64_t total = q * G.depth;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t k = (uint32_t)(t % G.depth); const uint64_t i = index_dev ? *index_dev : indices[t / G.depth];
    if (i >= m) continue;
    const uint64_t s = (i >> k) ^ 1;
    const uint8_t *src = ((s + 1) << k) <= m ? G.nodes + 32 * (tree_off(G.cap_log, k) + s) : (s << k) >= m ? G.empty + 32 * k : edge_bytes + 32 * k;
    tree_copy32(out + 64 + 32 * t, src);
  }
}
// the tree goes back to state m, 1 <= m < n: the edge is written to the level arrays and nothing else; nodes beyond the new counts stay as stale bytes that no kernel
// reads (k_tree_path and k_tree_append go by the counts)
__global__ void __launch_bounds__(64) k_tree_rewind(TreeGeom G, uint64_t m) {
  if (threadIdx.x) return;
  tree_edge_walk(G, m, [&](uint32_t k, const Node &B) { tree_store(G.nodes + 32 * (tree_off(G.cap_log, k) + ((m - 1) >> k)), B); });
}

// ---- anchors (DESIGN.md "A block against the resident tree") --------------------------------------------------------------------------------------------------
// match[t] = the lowest a < m with roots[a] == RT t, or -1.  roots are the m x 32 bytes that k_tree_roots_at wrote in an EARLIER launch (plain stores are not
// visible across XCDs inside one launch), in blob order; an RT comes in blob order or (hash_order) as the bytes of its common.Hash: blob word i is then word 7 - i
// with its bytes swapped, made once, in registers.  One lane a record; the roots pass through LDS in tiles of MATCH_TILE, a barrier before a tile is read and one
// before it is overwritten.  Inside a tile every lane walks the anchors in index order, eight a step: word 0 first — all lanes read one LDS address, a broadcast — and the other
// seven only where word 0 is equal; the lowest match stays.  A lane at or beyond q takes part in the tile loads and reaches every barrier; it compares and stores nothing.  No atomics.
constexpr int MATCH_THREADS = 256, MATCH_TILE = 256;
__global__ void __launch_bounds__(MATCH_THREADS) k_tree_match_roots(const uint32_t *__restrict__ roots, uint32_t m, const uint32_t *__restrict__ rts, uint64_t q, int hash_order,
                                                                    int32_t *__restrict__ match) {
  __shared__ uint32_t tile[8 * MATCH_TILE];
  const uint32_t tid = threadIdx.x; const uint64_t t = (uint64_t)blockIdx.x * MATCH_THREADS + tid; const bool live = t < q;
  uint32_t r[8];
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = 0;
  if (live) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = rts[8 * t + i];
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = hash_order ? __builtin_bswap32(w[7 - i]) : w[i];
  }
  int32_t best = -1;
#pragma unroll 1
  for (uint32_t base = 0; base < m; base += MATCH_TILE) {
    const uint32_t cnt = m - base < (uint32_t)MATCH_TILE ? m - base : (uint32_t)MATCH_TILE;    // (uniform: the barriers below are reached by every lane)
    __syncthreads();                                                                            // the tile before this one has been read by everyone
    for (uint32_t i = tid; i < 8 * cnt; i += MATCH_THREADS) tile[i] = roots[8 * (uint64_t)base + i];
    __syncthreads();
    if (live && best < 0) {
      // eight anchors a step: their words 0 are eight independent LDS reads in flight, where one read a step waits out the LDS latency 256 times a tile.  a + j stays
      // inside the tile whatever cnt is (a is a multiple of 8 below 256); an entry at or beyond cnt is stale and is not looked at.
#pragma unroll 1
      for (uint32_t a = 0; a < cnt && best < 0; a += 8) {
        uint32_t w0[8];
#pragma unroll
        for (int j = 0; j < 8; j++) w0[j] = tile[8 * (a + j)];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          if (best >= 0 || a + j >= cnt || w0[j] != r[0]) continue;
          bool same = true;
#pragma unroll
          for (int i = 1; i < 8; i++) same &= tile[8 * (a + j) + i] == r[i];
          if (same) best = (int32_t)(base + a + j);
        }
      }
    }
  }
  if (live) match[t] = best;
}
// k_tree_match_roots with a window a record (DESIGN.md "A stretch of the chain"): match[t] = the lowest a with lo[t] <= a < hi[t] and roots[a] == RT t, or -1.  The
// host has checked lo[t] <= hi[t] <= m.  Records come in block order, so the windows of one workgroup lie close together: the workgroup reduces min lo and max hi
// over its live lanes with a window that is not empty — inside a wave by shuffles, across the four waves through LDS, one barrier — and loads tiles only from
// floor(min lo / 8) * 8 up to max hi.  Both bounds are the same in every lane (made scalar below), so a lane at or beyond q, or one with an empty window, still
// reaches every barrier; a workgroup whose windows are all empty loads nothing.  A tile starts at a multiple of 8, so the steps of eight stay aligned with the
// tile; a lane starts at the step that holds its lo and skips what lies below lo or at and beyond hi.  Word 0 first, eight LDS reads a step, lowest index wins.
__global__ void __launch_bounds__(MATCH_THREADS) k_tree_match_roots_window(const uint32_t *__restrict__ roots, const uint32_t *__restrict__ rts, uint64_t q, const uint32_t *__restrict__ lo,
                                                                           const uint32_t *__restrict__ hi, int hash_order, int32_t *__restrict__ match) {
  __shared__ uint32_t tile[8 * MATCH_TILE]; __shared__ uint32_t ends[2 * (MATCH_THREADS / 64)];
  const uint32_t tid = threadIdx.x; const uint64_t t = (uint64_t)blockIdx.x * MATCH_THREADS + tid; const bool live = t < q;
  uint32_t r[8], my_lo = 0, my_hi = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = 0;
  if (live) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = rts[8 * t + i];
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = hash_order ? __builtin_bswap32(w[7 - i]) : w[i];
    my_lo = lo[t]; my_hi = hi[t];
  }
  const bool any = my_lo < my_hi;                                                                 // (false for a lane at or beyond q)
  uint32_t w_lo = any ? my_lo : 0xffffffffu, w_hi = any ? my_hi : 0u;
#pragma unroll
  for (int off = 32; off; off >>= 1) { const uint32_t a = __shfl_xor(w_lo, off), b = __shfl_xor(w_hi, off); w_lo = a < w_lo ? a : w_lo; w_hi = b > w_hi ? b : w_hi; }
  if ((tid & 63) == 0) { ends[tid >> 6] = w_lo; ends[MATCH_THREADS / 64 + (tid >> 6)] = w_hi; }
  __syncthreads();
  uint32_t g_lo = 0xffffffffu, g_hi = 0;
#pragma unroll
  for (int v = 0; v < MATCH_THREADS / 64; v++) { const uint32_t a = ends[v], b = ends[MATCH_THREADS / 64 + v]; g_lo = a < g_lo ? a : g_lo; g_hi = b > g_hi ? b : g_hi; }
  g_lo = __builtin_amdgcn_readfirstlane(g_lo); g_hi = __builtin_amdgcn_readfirstlane(g_hi);     // (every lane read the same eight words)
  int32_t best = -1;
#pragma unroll 1
  for (uint32_t base = g_lo < g_hi ? g_lo & ~7u : g_hi; base < g_hi; base += MATCH_TILE) {
    const uint32_t cnt = g_hi - base < (uint32_t)MATCH_TILE ? g_hi - base : (uint32_t)MATCH_TILE;  // (uniform; base + cnt <= max hi <= m: the loads stay inside roots)
    __syncthreads();                                                                            // the tile before this one has been read by everyone
    for (uint32_t i = tid; i < 8 * cnt; i += MATCH_THREADS) tile[i] = roots[8 * (uint64_t)base + i];
    __syncthreads();
    if (any && best < 0 && my_lo < base + cnt && my_hi > base) {
      const uint32_t a0 = my_lo > base ? (my_lo - base) & ~7u : 0u, a1 = my_hi - base < cnt ? my_hi - base : cnt;   // this lane's anchors of the tile: [max(a0, lo - base), a1)
#pragma unroll 1
      for (uint32_t a = a0; a < a1 && best < 0; a += 8) {
        uint32_t w0[8];
#pragma unroll
        for (int j = 0; j < 8; j++) w0[j] = tile[8 * (a + j)];                                    // (a is a multiple of 8 below 256: a + j stays inside the tile)
#pragma unroll
        for (int j = 0; j < 8; j++) {
          if (best >= 0 || base + a + j < my_lo || a + j >= a1 || w0[j] != r[0]) continue;
          bool same = true;
#pragma unroll
          for (int i = 1; i < 8; i++) same &= tile[8 * (a + j) + i] == r[i];
          if (same) best = (int32_t)(base + a + j);
        }
      }
    }
  }
  if (live) match[t] = best;
}

struct CommitmentTree::Impl {
  std::mutex mu; uint32_t depth = 0, cap_log = 0; uint64_t n = 0; DevBuf<uint8_t> nodes, empty, out, first /* k_tree_find's word */; std::vector<uint8_t> empty_host;
  uint64_t launches = 0, state_launches = 0; DevBuf<uint8_t> q_in, q_out;   // past states: the sizes or indices of a call, and its answer (kept and grown)
  // [root | index | q paths] of state m >= 1 in one download: the indices from the host or (from_find, q = 1) from k_tree_find's word
  void fetch_at(uint64_t m, const uint64_t *indices, size_t q, bool from_find, std::vector<uint8_t> &host) {
    hipStream_t s = gpu().stream; const size_t bytes = 64 + 32 * q * depth; grow_buf(q_out, bytes);
    if (!from_find && q) { grow_buf(q_in, 8 * q); HIP_CHECK(hipMemcpyAsync(q_in.get(), indices, 8 * q, hipMemcpyHostToDevice, s)); }
    const unsigned nb = (unsigned)std::min<uint64_t>(std::max<uint64_t>(cdiv(q * depth, 256), 1), 256);
    hipLaunchKernelGGL(k_tree_paths_at, dim3(nb), dim3(256), 0, s, geom(), m, from_find ? nullptr : (const unsigned long long *)q_in.get(),
                       from_find ? (const unsigned long long *)first.get() : nullptr, (uint64_t)q, q_out.get()); state_launches++;
    HIP_CHECK(hipGetLastError()); host.resize(bytes); q_out.download(host.data(), bytes);
  }
  TreeGeom geom() const { return TreeGeom{nodes.get(), empty.get(), cap_log, depth}; }
  static size_t bytes_for(uint32_t cap_log, uint32_t depth) { return 32 * (size_t)(tree_off(cap_log, depth) + 1); }
  // room for n_new leaves: a new allocation of twice the capacity or more, every level copied over by the library's copy kernel
  void reserve(uint64_t n_new) {
    if (n_new <= (1ull << cap_log)) return;
    uint32_t c = cap_log + 1; while ((1ull << c) < n_new) c++;
    DevBuf<uint8_t> fresh(bytes_for(c, depth));
    for (uint32_t k = 0; k <= depth && n; k++) { const uint64_t cnt = (n >> k) + ((n & ((1ull << k) - 1)) ? 1 : 0);
      copy_dev_async(fresh.get() + 32 * tree_off(c, k), nodes.get() + 32 * tree_off(cap_log, k), 32 * (size_t)cnt); }
    HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(gpu().stream));                  // (the old allocation is let go below)
    nodes = std::move(fresh); cap_log = c;
  }
  // [index | path | root] of the current state in one download; index_dev: take the index from k_tree_find's word
  void fetch(uint64_t index, bool index_from_find, std::vector<uint8_t> &host) {
    hipLaunchKernelGGL(k_tree_path, dim3(1), dim3(64), 0, gpu().stream, geom(), n, index, index_from_find ? (const unsigned long long *)first.get() : nullptr, out.get());
    HIP_CHECK(hipGetLastError()); host.resize(32 * (depth + 2)); out.download(host.data(), host.size());
  }
  void find_async(const uint8_t leaf[32], uint64_t n) {                                           // among the first n leaves
    HIP_CHECK(hipMemsetAsync(first.get(), 0xff, 8, gpu().stream)); if (!n) return;
    uint4 t[2]; memcpy(t, leaf, 32); const unsigned nb = (unsigned)std::min<uint64_t>(cdiv(n, 256), 2048);
    hipLaunchKernelGGL(k_tree_find, dim3(nb), dim3(256), 0, gpu().stream, (const uint4 *)nodes.get(), n, t[0], t[1], (unsigned long long *)first.get());
  }
};

CommitmentTree::CommitmentTree(int depth) : impl(new Impl) {
  if (depth < 1 || depth > 32) throw GpuError("commitment tree: the depth must lie between 1 and 32");
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); Impl &d = *impl; d.depth = (uint32_t)depth; d.cap_log = std::min<uint32_t>(TREE_MIN_CAP_LOG, d.depth);
  d.empty_host.assign(32 * (depth + 1), 0);
  for (int k = 1; k <= depth; k++) sha256_compress_raw(&d.empty_host[32 * (k - 1)], &d.empty_host[32 * (k - 1)], &d.empty_host[32 * k]);
  d.nodes = DevBuf<uint8_t>(Impl::bytes_for(d.cap_log, d.depth)); d.empty = DevBuf<uint8_t>(d.empty_host.size()); d.out = DevBuf<uint8_t>(32 * (depth + 2));
  d.first = DevBuf<uint8_t>(8); d.empty.upload(d.empty_host.data(), d.empty_host.size());
}
CommitmentTree::~CommitmentTree() { try { LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); impl.reset(); } catch (...) {} }
int CommitmentTree::depth() const { return (int)impl->depth; }
uint64_t CommitmentTree::size() const { std::lock_guard<std::mutex> lk(impl->mu); return impl->n; }
uint64_t CommitmentTree::launches() const { std::lock_guard<std::mutex> lk(impl->mu); return impl->launches; }
uint64_t CommitmentTree::state_launches() const { std::lock_guard<std::mutex> lk(impl->mu); return impl->state_launches; }

bool CommitmentTree::append(const uint8_t *leaves, size_t count) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if (count > (1ull << d.depth) - d.n) return false;
  if (!count) return true;
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream;
  const uint64_t n_old = d.n, n_new = d.n + count; d.reserve(n_new);
  { Stage up("tree.upload"); HIP_CHECK(hipMemcpyAsync(d.nodes.get() + 32 * n_old, leaves, 32 * count, hipMemcpyHostToDevice, s)); }
  // tiled launches while the dirty range of the base level is wider than one window, then the ragged one to the root
  { Stage st("tree.append");                                                                     // (HIP events when profiling is on: tools/tree_bench.py)
  for (uint32_t k0 = 0;;) {
    const uint64_t lo = n_old >> k0, hi = (n_new >> k0) + ((n_new & ((1ull << k0) - 1)) ? 1 : 0);
    if (hi - lo <= TREE_TILE || k0 + TREE_TILE_LOG >= d.depth) {
      // (a base level that is too wide can only be left here if depth - k0 <= TREE_TILE_LOG, and then 2^depth >> k0 <= TREE_TILE bounds it: never)
      hipLaunchKernelGGL(k_tree_append, dim3(1), dim3(TREE_THREADS), 0, s, d.geom(), n_old, n_new, k0, d.depth - k0, (uint64_t)0, 1); d.launches++;
      break;
    }
    const uint64_t t0 = lo >> TREE_TILE_LOG, t1 = (hi - 1) >> TREE_TILE_LOG;
    hipLaunchKernelGGL(k_tree_append, dim3((unsigned)(t1 - t0 + 1)), dim3(TREE_THREADS), 0, s, d.geom(), n_old, n_new, k0, (uint32_t)TREE_TILE_LOG, t0, 0); d.launches++;
    k0 += TREE_TILE_LOG;
  } }
  HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(s));
  d.n = n_new; return true;
}
void CommitmentTree::root(uint8_t out[32]) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if (!d.n) { memcpy(out, &d.empty_host[32 * d.depth], 32); return; }
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream;
  HIP_CHECK(hipMemcpyAsync(out, d.nodes.get() + 32 * tree_off(d.cap_log, d.depth), 32, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
}
bool CommitmentTree::path(uint64_t index, uint8_t *siblings) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu); if (index >= d.n) return false;
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); std::vector<uint8_t> h; d.fetch(index, false, h);
  memcpy(siblings, h.data() + 32, 32 * d.depth); return true;
}
bool CommitmentTree::find(const uint8_t leaf[32], uint64_t &index) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu); if (!d.n) return false;
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); d.find_async(leaf, d.n); HIP_CHECK(hipGetLastError());
  uint64_t got = 0; d.first.download((uint8_t *)&got, 8); if (got >= d.n) return false;
  index = got; return true;
}
bool CommitmentTree::snapshot(const uint8_t leaf[32], Snapshot &out) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu); out.size = d.n; out.path.assign(32 * d.depth, 0); out.index_bits.assign(d.depth, false); out.index = 0;
  if (!d.n) { memcpy(out.root, &d.empty_host[32 * d.depth], 32); return false; }
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); std::vector<uint8_t> h; d.find_async(leaf, d.n); d.fetch(0, true, h);   // find, gather, one download
  memcpy(out.root, h.data() + 32 * (d.depth + 1), 32);
  uint64_t got; memcpy(&got, h.data(), 8); if (got >= d.n) return false;
  out.index = got; memcpy(out.path.data(), h.data() + 32, 32 * d.depth);
  for (uint32_t k = 0; k < d.depth; k++) out.index_bits[k] = (got >> k) & 1;
  return true;
}

// ---- past states: every entry checks its arguments before anything is queued, so a failing call writes nothing and changes nothing ----------------------------
bool CommitmentTree::roots_at(const uint64_t *sizes, size_t q, uint8_t *out) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if (q && (!sizes || !out)) return false;
  for (size_t i = 0; i < q; i++) if (sizes[i] > d.n) return false;
  if (!q) return true;
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream;
  grow_buf(d.q_in, 8 * q); grow_buf(d.q_out, 32 * q); std::vector<uint8_t> h(32 * q); SyncAtExit sync;   // (the vector outlives the synchronise)
  HIP_CHECK(hipMemcpyAsync(d.q_in.get(), sizes, 8 * q, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_tree_roots_at, dim3((unsigned)cdiv(q, 64)), dim3(64), 0, s, d.geom(), (const unsigned long long *)d.q_in.get(), (uint64_t)q, d.q_out.get()); d.state_launches++;
  HIP_CHECK(hipGetLastError()); d.q_out.download(h.data(), h.size());
  memcpy(out, h.data(), h.size()); return true;
}
// The anchor step of a block: one upload [sizes | RTs], k_tree_roots_at as it is — its roots stay in device memory —, then k_tree_match_roots in a launch of its
// own, which is what makes the roots visible to it, and q x 4 bytes back.
bool CommitmentTree::match_roots(const uint64_t *sizes, size_t m, const uint8_t *rts, size_t q, bool hash_order, int32_t *match_out) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if ((m && !sizes) || (q && (!rts || !match_out)) || m >= (1ull << 31)) return false;
  for (size_t i = 0; i < m; i++) if (sizes[i] > d.n) return false;
  if (!q) return true;
  if (!m) { for (size_t i = 0; i < q; i++) match_out[i] = -1; return true; }
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream;
  std::vector<uint8_t> up(8 * m + 32 * q); memcpy(up.data(), sizes, 8 * m); memcpy(up.data() + 8 * m, rts, 32 * q);
  grow_buf(d.q_in, up.size()); grow_buf(d.q_out, 32 * m + 4 * q); std::vector<int32_t> h(q); SyncAtExit sync;   // (the vectors outlive the synchronise)
  HIP_CHECK(hipMemcpyAsync(d.q_in.get(), up.data(), up.size(), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_tree_roots_at, dim3((unsigned)cdiv(m, 64)), dim3(64), 0, s, d.geom(), (const unsigned long long *)d.q_in.get(), (uint64_t)m, d.q_out.get()); d.state_launches++;
  hipLaunchKernelGGL(k_tree_match_roots, dim3((unsigned)cdiv(q, MATCH_THREADS)), dim3(MATCH_THREADS), 0, s, (const uint32_t *)d.q_out.get(), (uint32_t)m,
                     (const uint32_t *)(d.q_in.get() + 8 * m), (uint64_t)q, hash_order ? 1 : 0, (int32_t *)(d.q_out.get() + 32 * m)); d.state_launches++;
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(h.data(), d.q_out.get() + 32 * m, 4 * q, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  memcpy(match_out, h.data(), 4 * q); return true;
}
// match_roots with a window a record: one upload [sizes | RTs | lo | hi], the same two launches with k_tree_match_roots_window as the second, q x 4 bytes back.
// The windows are checked here, under the tree's lock and before anything is queued: the kernel trusts lo <= hi <= m.
bool CommitmentTree::match_roots_window(const uint64_t *sizes, size_t m, const uint8_t *rts, size_t q, const uint32_t *lo, const uint32_t *hi, bool hash_order, int32_t *match_out) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if ((m && !sizes) || (q && (!rts || !lo || !hi || !match_out)) || m >= (1ull << 31)) return false;
  for (size_t i = 0; i < m; i++) if (sizes[i] > d.n) return false;
  for (size_t i = 0; i < q; i++) if (lo[i] > hi[i] || hi[i] > m) return false;
  if (!q) return true;
  if (!m) { for (size_t i = 0; i < q; i++) match_out[i] = -1; return true; }
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream;
  const size_t at_rts = 8 * m, at_lo = at_rts + 32 * q, at_hi = at_lo + 4 * q;                   // (8 m and 32 q keep the words aligned)
  std::vector<uint8_t> up(at_hi + 4 * q); memcpy(up.data(), sizes, 8 * m); memcpy(up.data() + at_rts, rts, 32 * q); memcpy(up.data() + at_lo, lo, 4 * q); memcpy(up.data() + at_hi, hi, 4 * q);
  grow_buf(d.q_in, up.size()); grow_buf(d.q_out, 32 * m + 4 * q); std::vector<int32_t> h(q); SyncAtExit sync;   // (the vectors outlive the synchronise)
  HIP_CHECK(hipMemcpyAsync(d.q_in.get(), up.data(), up.size(), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_tree_roots_at, dim3((unsigned)cdiv(m, 64)), dim3(64), 0, s, d.geom(), (const unsigned long long *)d.q_in.get(), (uint64_t)m, d.q_out.get()); d.state_launches++;
  hipLaunchKernelGGL(k_tree_match_roots_window, dim3((unsigned)cdiv(q, MATCH_THREADS)), dim3(MATCH_THREADS), 0, s, (const uint32_t *)d.q_out.get(), (const uint32_t *)(d.q_in.get() + at_rts),
                     (uint64_t)q, (const uint32_t *)(d.q_in.get() + at_lo), (const uint32_t *)(d.q_in.get() + at_hi), hash_order ? 1 : 0, (int32_t *)(d.q_out.get() + 32 * m)); d.state_launches++;
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(h.data(), d.q_out.get() + 32 * m, 4 * q, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  memcpy(match_out, h.data(), 4 * q); return true;
}
bool CommitmentTree::paths_at(uint64_t size, const uint64_t *indices, size_t q, uint8_t *siblings, uint8_t *root) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu);
  if (size > d.n || (q && (!indices || !siblings))) return false;
  for (size_t i = 0; i < q; i++) if (indices[i] >= size) return false;
  if (!size) { if (root) memcpy(root, &d.empty_host[32 * d.depth], 32); return true; }          // (q = 0 here: no index lies below 0)
  if (!q && !root) return true;
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); std::vector<uint8_t> h; SyncAtExit sync; d.fetch_at(size, indices, q, false, h);
  if (q) memcpy(siblings, h.data() + 64, 32 * q * d.depth);
  if (root) memcpy(root, h.data(), 32);
  return true;
}
bool CommitmentTree::find_at(uint64_t size, const uint8_t leaf[32], uint64_t &index) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu); if (size > d.n || !leaf || !size) return false;
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); uint64_t got = 0; SyncAtExit sync; d.find_async(leaf, size); d.state_launches++; HIP_CHECK(hipGetLastError());
  d.first.download((uint8_t *)&got, 8); if (got >= size) return false;
  index = got; return true;
}
bool CommitmentTree::snapshot_at(uint64_t size, const uint8_t leaf[32], Snapshot &out) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu); out.size = size; out.path.assign(32 * d.depth, 0); out.index_bits.assign(d.depth, false); out.index = 0;
  memcpy(out.root, &d.empty_host[32 * d.depth], 32);
  if (size > d.n || !size || !leaf) return false;                                                 // (a size the tree does not hold: the empty root, and false)
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); std::vector<uint8_t> h; SyncAtExit sync;
  d.find_async(leaf, size); d.state_launches++; d.fetch_at(size, nullptr, 1, true, h);            // find, edge walk and gather, one download
  memcpy(out.root, h.data(), 32);
  uint64_t got; memcpy(&got, h.data() + 32, 8); if (got >= size) return false;
  out.index = got; memcpy(out.path.data(), h.data() + 64, 32 * d.depth);
  for (uint32_t k = 0; k < d.depth; k++) out.index_bits[k] = (got >> k) & 1;
  return true;
}
bool CommitmentTree::rewind(uint64_t size) {
  Impl &d = *impl; std::lock_guard<std::mutex> lk(d.mu); if (size > d.n) return false;
  if (size == d.n) return true;
  if (!size) { d.n = 0; return true; }                                                            // the empty tree reads no node
  LaneScope lane(0); std::lock_guard<std::mutex> gl(g_gpu_mutex); hipStream_t s = gpu().stream;
  hipLaunchKernelGGL(k_tree_rewind, dim3(1), dim3(64), 0, s, d.geom(), size); d.state_launches++;
  HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(s));
  d.n = size; return true;
}

}  // namespace zk
