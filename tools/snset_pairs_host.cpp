// The host side of tools/snset_pairs_bench.py: the node's check with up to two keys a record as a program would write it on one core — a std::unordered_set of
// 20-byte keys, and for each record in order: Exist on each key, then CreateAccount on each (core/state_processor.go:106-179).  Built by the tool with
// g++ -O2 -shared -fPIC.  Stateful, as tools/snset_host.cpp is, so that a call costs what the loop costs and not the set's construction.
#include <cstdint>
#include <cstring>
#include <unordered_set>
#include <vector>
struct Key { uint32_t w[5]; bool operator==(const Key &o) const { return !memcmp(w, o.w, 20); } };
struct KeyHash { size_t operator()(const Key &k) const { uint64_t h = 0x9E3779B97F4A7C15ull; for (int i = 0; i < 5; i++) { h = (h ^ k.w[i]) * 0xD6E8FEB86659FD93ull; h ^= h >> 32; } return (size_t)h; } };
struct HostSet { std::unordered_set<Key, KeyHash> s; std::vector<Key> last; };
extern "C" {
HostSet *hostpairs_new(void) { return new HostSet; }
void hostpairs_free(HostSet *h) { delete h; }
uint64_t hostpairs_size(HostSet *h) { return h->s.size(); }
// keys: n x 2 x 20 bytes, nkeys[i] = 0, 1 or 2.  conflict[i] = 1 if a key of record i is in the set (the keys of the earlier accepted records of the call included, as
// they were inserted) or its two keys are equal; otherwise the record's keys are inserted.  A rejected record inserts nothing.
void hostpairs_spend(HostSet *h, const uint8_t *keys, const uint8_t *nkeys, uint64_t n, uint8_t *conflict) {
  h->last.clear();
  for (uint64_t i = 0; i < n; i++) {
    Key k[2]; const unsigned m = nkeys[i]; bool taken = false;
    for (unsigned j = 0; j < m; j++) { memcpy(k[j].w, keys + 40 * i + 20 * j, 20); taken = taken || h->s.count(k[j]) != 0; }
    if (m == 2 && k[0] == k[1]) taken = true;
    conflict[i] = taken;
    if (!taken) for (unsigned j = 0; j < m; j++) { h->s.insert(k[j]); h->last.push_back(k[j]); }
  }
}
void hostpairs_undo(HostSet *h) { for (const Key &k : h->last) h->s.erase(k); h->last.clear(); }   // outside the clock: the set goes back to what it was before the last call
}
