// SplitLayout and PackedLayout (blockmaze_amd/csrc/txs_layout.hpp) as a program of its own, for the sanitizer build that tests/test_raw_bodies_cpu.py
// makes, in the manner of tests/txs_layout_driver.cpp.  Over a sweep of block counts, byte totals and caps every layout is held to its structure — the regions
// ascend, do not overlap and end inside the buffer; what a kernel reads or writes as 64-bit words stands at an even word; the mid-call download is one range and ends
// where tx_beg starts — and to the formulas of the header's description, restated here with literals.  Then the layout is used as the host uses it: a buffer of exactly
// its size is filled region by region and read back, so that a region that leaves the buffer is the sanitizer's to find.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "txs_layout.hpp"

using namespace zk;
static int fails = 0; static char ctx[160];
static void eq(const char *what, size_t got, size_t want) { if (got != want && fails++ < 20) printf("%s: %s is %zu, expected %zu\n", ctx, what, got, want); }
static void even(const char *what, size_t x) { if ((x & 1) && fails++ < 20) printf("%s: %s = %zu is not 8-byte aligned\n", ctx, what, x); }
static size_t up8(size_t v) { return (v + 7) / 8 * 8; }
struct Region { const char *name; size_t at, words; };

static void split(size_t nb, size_t total, size_t cap) {
  snprintf(ctx, sizeof ctx, "SplitLayout(%zu, %zu, %zu)", nb, total, cap); const SplitLayout L = split_layout(nb, total, cap);
  const size_t tx_cap = cap < total ? cap : total, up = up8(total) + 8 * (nb + 1), stw = (nb + 3) / 4;
  const size_t pay_beg = up / 4, pay_size = pay_beg + nb, count = pay_size + nb, base = (count + nb + 1) / 2 * 2, head = base + 2 * (nb + 1), first = head + 8, status = first + nb + 1;
  const size_t tx_beg = (status + stw + 1) / 2 * 2, tx_size = tx_beg + 2 * tx_cap, end = (tx_size + tx_cap + 1) / 2 * 2;
  eq("total", L.total, total); eq("total8", L.total8, up8(total)); eq("up", L.up, up); eq("body_off", 4 * L.body_off, up8(total)); eq("tx_cap", L.tx_cap, tx_cap);
  eq("pay_beg", L.pay_beg, pay_beg); eq("pay_size", L.pay_size, pay_size); eq("count", L.count, count); eq("base", L.base, base); eq("head", L.head, head); eq("down", L.down, head);
  eq("first", L.first, first); eq("status", L.status, status); eq("tx_beg", L.tx_beg, tx_beg); eq("tx_size", L.tx_size, tx_size); eq("end", L.end, end);
  eq("the pinned total", L.pin_bytes, up + 4 * (end - head)); eq("the mid-call download", 4 * (L.tx_beg - L.down), 4 * (tx_beg - head));
  even("body_off", L.body_off); even("base", L.base); even("head", L.head); even("tx_beg", L.tx_beg); even("end", L.end); eq("up mod 8", L.up % 8, 0);
  const std::vector<Region> r = {{"body_off", L.body_off, 2 * (nb + 1)}, {"pay_beg", L.pay_beg, nb}, {"pay_size", L.pay_size, nb}, {"count", L.count, nb}, {"base", L.base, 2 * (nb + 1)},
                                 {"head", L.head, TXL_SPLIT_HEAD}, {"first", L.first, nb + 1}, {"status", L.status, stw}, {"tx_beg", L.tx_beg, 2 * tx_cap}, {"tx_size", L.tx_size, tx_cap}};
  size_t at = (total + 3) / 4;
  for (const Region &x : r) { if (x.at < at && fails++ < 20) printf("%s: %s at %zu starts before %zu, where the region before it ends\n", ctx, x.name, x.at, at); at = x.at + x.words; }
  if (at > L.end && fails++ < 20) printf("%s: the last region ends at %zu, behind end = %zu\n", ctx, at, L.end);
  // as the host uses it: the device buffer with its slack, and the pinned buffer with the upload in front and region x of the download at up + 4 (x - down)
  std::vector<uint32_t> dev(L.end + TXL_SLACK, 0); std::vector<uint8_t> pin(L.pin_bytes, 0); uint32_t tag = 1;
  memset(pin.data(), 0xEE, L.total); memset(pin.data() + L.total, 0, L.total8 - L.total); memset(pin.data() + L.total8, 0x11, 8 * (nb + 1));
  memcpy(dev.data(), pin.data(), L.up);
  for (const Region &x : r) { if (x.at == L.body_off) continue; for (size_t k = 0; k < x.words; k++) dev[x.at + k] = tag; tag++; }
  memcpy(pin.data() + L.up, dev.data() + L.down, 4 * (L.tx_beg - L.down));
  if (tx_cap) { memcpy(pin.data() + L.up + 4 * (L.tx_beg - L.down), dev.data() + L.tx_beg, 8 * tx_cap); memcpy(pin.data() + L.up + 4 * (L.tx_size - L.down), dev.data() + L.tx_size, 4 * tx_cap); }
  tag = 1;
  for (const Region &x : r) { if (x.at == L.body_off) continue;
    for (size_t k = 0; k < x.words; k++) if (dev[x.at + k] != tag && fails++ < 20) printf("%s: word %zu of %s was overwritten by a later region\n", ctx, k, x.name);
    if (x.at >= L.down) { uint32_t v = tag; if (x.words && memcmp(pin.data() + L.up + 4 * (x.at - L.down), &v, 4) != 0 && fails++ < 20) printf("%s: %s does not land where the host reads it\n", ctx, x.name); }
    tag++; }
  for (size_t k = 0; k < 2 * (nb + 1); k++) if (dev[L.body_off + k] != 0x11111111u && fails++ < 20) printf("%s: body_off was overwritten\n", ctx);
}
static void packed(size_t n, size_t total, size_t nb) {
  snprintf(ctx, sizeof ctx, "PackedLayout(%zu, %zu, %zu)", n, total, nb); const PackedLayout L = packed_layout(n, total, nb);
  const size_t up = up8(total) + 8 * (n + 1) + up8(4 * (nb + 1));
  eq("up", L.up, up); eq("off", 4 * L.off, up8(total)); eq("first", 4 * L.first, up8(total) + 8 * (n + 1)); eq("n_first", L.n_first, nb + 1); eq("down", L.down, 0); eq("the download", 4 * (L.down_end - L.down), up);
  eq("the device total", L.end + TXL_SLACK, up / 4 + 2); eq("the pinned total", L.pin_bytes, 2 * up); even("off", L.off); even("first", L.first);
}

int main() {
  std::vector<size_t> nbs, totals; size_t layouts = 0;
  for (size_t n = 0; n <= 9; n++) nbs.push_back(n);
  for (size_t n : {63, 64, 65, 255, 256, 257, 4097}) nbs.push_back(n);
  for (size_t t = 0; t < 8; t++) { totals.push_back(t); totals.push_back(8 + t); totals.push_back(1000 + t); }   // every residue mod 8
  for (size_t nb : nbs) for (size_t total : totals) for (size_t cap : {(size_t)0, (size_t)1, (size_t)7, total / 2, total, total + 1, (size_t)1 << 31}) {
    split(nb, total, cap); packed(cap < total ? cap : total, total, nb); layouts += 2; }
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("SPLIT LAYOUT OK: %zu layouts\n", layouts);
  return 0;
}
