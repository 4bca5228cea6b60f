// The host comparand of tools/accounts_bench.py: the loop a node runs today before it can call verifyBlockTree, and after the block is accepted — one
// std::unordered_map from address to balance commitment, walked once a record in order on one core:
//     old := map[from] (zero hash if absent), written into the record's old slot;  map[from] := the record's new slot.
// A journal of (address, previous value, was present) an update makes the rewind of a reorganisation possible, as the account table's log does.
//     g++ -O2 -shared -fPIC tools/accounts_host.cpp -o tools/accounts_host.so
#include <array>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

namespace {
typedef std::array<uint8_t, 20> Addr; typedef std::array<uint8_t, 32> Val;
struct Hash { size_t operator()(const Addr &a) const { uint64_t h; memcpy(&h, a.data() + 12, 8); return (size_t)(h * 0x9E3779B97F4A7C15ull); } };
struct Undo { Addr a; Val v; bool had; };
struct Table { std::unordered_map<Addr, Val, Hash> map; std::vector<Undo> journal; };
const size_t REC = 720, ARGS = 528;
inline int old_arg(uint8_t kind) { return kind == 2 ? 2 : 0; }
inline int new_arg(uint8_t kind) { return kind == 2 ? 4 : kind == 1 ? 3 : 2; }
inline void put(Table &t, const Addr &a, const uint8_t *v) {
  auto it = t.map.find(a); Undo u; u.a = a; u.had = it != t.map.end(); if (u.had) u.v = it->second; else u.v.fill(0);
  t.journal.push_back(u); Val nv; memcpy(nv.data(), v, 32); if (u.had) it->second = nv; else t.map.emplace(a, nv);
}
}

extern "C" {
void *accounts_host_new(void) { return new Table; }
void accounts_host_free(void *h) { delete (Table *)h; }
uint64_t accounts_host_size(void *h) { return ((Table *)h)->journal.size(); }
void accounts_host_set(void *h, const uint8_t *addrs, const uint8_t *values, size_t n) {
  Table &t = *(Table *)h; t.map.reserve(t.map.size() + n);
  for (size_t i = 0; i < n; i++) { Addr a; memcpy(a.data(), addrs + 20 * i, 20); put(t, a, values + 32 * i); }
}
// the chained fill and the commit of one accepted block, in one pass as a node's state processor makes it
void accounts_host_block(void *h, const uint8_t *froms, uint8_t *recs, size_t n) {
  Table &t = *(Table *)h;
  for (size_t i = 0; i < n; i++) {
    uint8_t *r = recs + REC * i; if (r[0] > 3) continue;
    Addr a; memcpy(a.data(), froms + 20 * i, 20); auto it = t.map.find(a);
    if (it != t.map.end()) memcpy(r + ARGS + 32 * old_arg(r[0]), it->second.data(), 32); else memset(r + ARGS + 32 * old_arg(r[0]), 0, 32);
    put(t, a, r + ARGS + 32 * new_arg(r[0]));
  }
}
void accounts_host_rewind(void *h, uint64_t size) {
  Table &t = *(Table *)h;
  while (t.journal.size() > size) { const Undo &u = t.journal.back(); if (u.had) t.map[u.a] = u.v; else t.map.erase(u.a); t.journal.pop_back(); }
}
}
