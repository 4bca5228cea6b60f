// The host side of tools/snset_bench.py: the node's check as a program would write it on one core — a std::unordered_set of 20-byte keys, check-then-insert in record order.
// Built by the tool with g++ -O2 -shared -fPIC.  Stateful, unlike zkgpu_test_snset_host, so that a call costs what the loop costs and not the set's construction.
#include <cstdint>
#include <cstring>
#include <unordered_set>
#include <vector>
struct Key { uint32_t w[5]; bool operator==(const Key &o) const { return !memcmp(w, o.w, 20); } };
struct KeyHash { size_t operator()(const Key &k) const { uint64_t h = 0x9E3779B97F4A7C15ull; for (int i = 0; i < 5; i++) { h = (h ^ k.w[i]) * 0xD6E8FEB86659FD93ull; h ^= h >> 32; } return (size_t)h; } };
struct HostSet { std::unordered_set<Key, KeyHash> s; std::vector<Key> last; };
extern "C" {
HostSet *hostset_new(void) { return new HostSet; }
void hostset_free(HostSet *h) { delete h; }
uint64_t hostset_size(HostSet *h) { return h->s.size(); }
// conflict[i] = 1 if keys[i] is in the set (a repeat inside the call included, since the earlier one was inserted); commit: insert
void hostset_spend(HostSet *h, const uint8_t *keys, uint64_t n, int commit, uint8_t *conflict) {
  h->last.clear();
  for (uint64_t i = 0; i < n; i++) { Key k; memcpy(k.w, keys + 20 * i, 20);
    if (commit) { const bool fresh = h->s.insert(k).second; conflict[i] = !fresh; if (fresh) h->last.push_back(k); }
    else conflict[i] = h->s.count(k) != 0; }
}
void hostset_undo(HostSet *h) { for (const Key &k : h->last) h->s.erase(k); h->last.clear(); }   // outside the clock: the set goes back to what it was before the last call
void hostset_query(HostSet *h, const uint8_t *keys, uint64_t q, uint8_t *in) { for (uint64_t i = 0; i < q; i++) { Key k; memcpy(k.w, keys + 20 * i, 20); in[i] = h->s.count(k) != 0; } }
}
