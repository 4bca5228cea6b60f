// The workspace layouts of the transaction calls (blockmaze_amd/csrc/txs_layout.hpp) as a program of its own, for the sanitizer build that tests/test_txs_cpu.py
// makes.  Over a sweep of n, byte totals, list counts and flags, every layout is held to two things.  Its structure: the regions ascend, do not overlap and end inside
// the workspace; the download is one range of it; what a kernel reads or writes as 64-bit words stands at an even word.  And the numbers the four host functions of
// gpu_txs.hip were first written with — the upload, each download, the pinned and the device total, where each output lies in the download —, restated here as
// they stood there: a layout that yields another number has moved a region or a byte that crosses the bus.  This is the one place those literals live.
#include <cstddef>
#include <cstdio>
#include <vector>
#include "txs_layout.hpp"

using namespace zk;
static int fails = 0; static char ctx[160];
static void eq(const char *what, size_t got, size_t want) { if (got != want && fails++ < 20) printf("%s: %s is %zu, was %zu\n", ctx, what, got, want); }
static void even(const char *what, size_t x) { if ((x & 1) && fails++ < 20) printf("%s: %s = %zu is not 8-byte aligned\n", ctx, what, x); }
struct Region { const char *name; size_t at, words; };
// ascending, disjoint, inside end; down .. down_end starts at a region, ends at one and lies inside the workspace
static void structure(const TxsUpload &L, const std::vector<Region> &r) {
  size_t at = 0; bool down_starts = false, down_ends = L.down_end == L.down;
  for (const Region &x : r) {
    if (x.at < at && fails++ < 20) printf("%s: %s at %zu starts before %zu, where the region before it ends\n", ctx, x.name, x.at, at);
    at = x.at + x.words; down_starts |= x.at == L.down; down_ends |= at == L.down_end;
  }
  if (at > L.end && fails++ < 20) printf("%s: the last region ends at %zu, behind end = %zu\n", ctx, at, L.end);
  if ((!down_starts || !down_ends || L.down > L.down_end || L.down_end > L.end) && fails++ < 20) printf("%s: the download %zu .. %zu is no range of regions inside %zu\n", ctx, L.down, L.down_end, L.end);
  if (L.pin_bytes < L.up + 4 * (L.down_end - L.down) && fails++ < 20) printf("%s: the pinned buffer does not hold the upload and the download\n", ctx);
  even("off", L.off); even("first", L.first); even("the upload's end", L.up / 4); eq("up mod 8", L.up % 8, 0);
}
static size_t host(const TxsUpload &L, size_t x) { return 4 * (x - L.down); }   // the byte offset behind `back`

// ---- the formulas as the host functions had them -------------------------------------------------------------------------------------------------------------------
static size_t up8(size_t v) { return (v + 7) / 8 * 8; }
struct WasTrie { size_t blk_of, bad, node, roots, defined, end; };
static WasTrie was_trie(size_t base, size_t n, size_t n_lists) {
  WasTrie w; w.blk_of = base; w.bad = w.blk_of + n; w.node = (w.bad + n_lists + 1) / 2 * 2; w.roots = w.node + 8 * n; w.defined = w.roots + 8 * n_lists; w.end = w.defined + (n_lists + 7) / 8 * 2; return w;
}
static void eq_trie(const TrieWords &t, const WasTrie &w) {
  eq("blk_of", t.blk_of, w.blk_of); eq("bad", t.bad, w.bad); eq("node", t.node, w.node); eq("roots", t.roots, w.roots); eq("defined", t.defined, w.defined); eq("the trie's end", t.end, w.end);
  even("node", t.node); even("roots", t.roots);
}
static void eq_upload(const TxsUpload &L, size_t n, size_t total, size_t n_first) {
  const size_t up = up8(total) + 8 * (n + 1) + up8(4 * n_first), total8 = up - 8 * (n + 1) - up8(4 * n_first);
  eq("up", L.up, up); eq("total", L.total, total); eq("total8", L.total8, total8); eq("off", 4 * L.off, total8); eq("first", 4 * L.first, total8 + 8 * (n + 1)); eq("n_first", L.n_first, n_first);
}

static void sender_inputs(size_t n, size_t total) {
  snprintf(ctx, sizeof ctx, "SenderInputsLayout(%zu, %zu)", n, total); const SenderInputsLayout L = sender_inputs_layout(n, total);
  const size_t okw = (n + 3) / 4, down_words = 21 * n + (65 * n + 3) / 4 + 2 * okw + 4, down = 4 * down_words, up = up8(total) + 8 * (n + 1);
  const size_t w_up = up / 4, w_D = 9 * n, w_rec = 4 + okw + 5 * n, words = w_up + w_D + 24 * n + okw + w_rec + down_words + 2;
  const size_t D = w_up, hash = D + w_D, rs = hash + 8 * n, v = rs + 16 * n, rec = v + okw, dn = rec + w_rec;
  structure(L, {{"D", L.D, 9 * n}, {"hash", L.hash, 8 * n}, {"rs", L.rs, 16 * n}, {"v", L.v, okw}, {"rec", L.rec, 4}, {"ok", L.ok, okw}, {"recovered", L.recovered, 5 * n}, {"txhash", L.txhash, 8 * n},
                {"sighash", L.sighash, 8 * n}, {"froms", L.froms, 5 * n}, {"sigs", L.sigs, (65 * n + 3) / 4}, {"status", L.status, okw}, {"code", L.code, okw}, {"head", L.head, 4}});
  eq_upload(L, n, total, 0); eq("the device total", L.end + TXL_SLACK, words); eq("the pinned total", L.pin_bytes, up + down); eq("the download", 4 * (L.down_end - L.down), down);
  eq("D", L.D, D); eq("hash", L.hash, hash); eq("rs", L.rs, rs); eq("v", L.v, v); eq("rec", L.rec, rec); eq("ok", L.ok, rec + 4); eq("recovered", L.recovered, rec + 4 + okw); eq("down", L.down, dn);
  eq("txhash", L.txhash, dn); eq("sighash", L.sighash, dn + 8 * n); eq("froms", L.froms, dn + 16 * n); eq("sigs", L.sigs, dn + 21 * n); eq("status", 4 * L.status, 4 * (dn + 21 * n) + 4 * ((65 * n + 3) / 4));
  eq("code", 4 * L.code, 4 * (dn + 21 * n) + 4 * ((65 * n + 3) / 4) + 4 * okw); eq("head", L.head, dn + down_words - 4);
  eq("txhash in the download", host(L, L.txhash), 0); eq("sighash in the download", host(L, L.sighash), 32 * n); eq("froms in the download", host(L, L.froms), 64 * n);
  eq("sigs in the download", host(L, L.sigs), 84 * n); eq("status in the download", host(L, L.status), 84 * n + 4 * ((65 * n + 3) / 4));
  eq("code in the download", host(L, L.code), 84 * n + 4 * ((65 * n + 3) / 4) + 4 * okw); eq("head in the download", host(L, L.head), down - 16);
}

static void records(size_t n, size_t total, size_t n_blocks) {
  snprintf(ctx, sizeof ctx, "RecordsLayout(%zu, %zu, %zu)", n, total, n_blocks); const RecordsLayout L = records_layout(n, total, n_blocks); const bool roots = n_blocks != 0;
  const size_t BH_WORDS = 4, REC_WORDS = 180, TD_WORDS = 9, TE_WORDS = 10;
  const size_t okw = (n + 3) / 4, nb = (n + 127) / 128, small_words = (2 * BH_WORDS + 20 * n + 1 + 2 * okw + 1) / 2 * 2, down_words = small_words + REC_WORDS * n;
  const size_t n_first = roots ? n_blocks + 1 : 0, roots_down = roots ? 32 * n_blocks + up8(n_blocks) : 0, up = up8(total) + 8 * (n + 1) + up8(4 * n_first);
  const size_t w_up = up / 4, w_D = TD_WORDS * n, w_E = TE_WORDS * n, w_rec = 4 + okw + 5 * n, before = (w_up + w_D + w_E + 40 * n + okw + w_rec + n + 2 * nb + 1) / 2 * 2;
  const WasTrie tw = was_trie((before + down_words + 1) / 2 * 2, roots ? n : 0, roots ? n_blocks : 0);
  const size_t D = w_up, E = D + w_D, hash = E + w_E, rs = hash + 8 * n, xy = rs + 16 * n, v = xy + 16 * n, rec = v + okw, src_of = rec + w_rec, counts = src_of + n, bases = counts + nb, dn = before;
  const size_t d_txhash = dn + 2 * BH_WORDS, d_froms = d_txhash + 8 * n, d_rec_froms = d_froms + 5 * n, d_rec_of = d_rec_froms + 5 * n, d_prefix = d_rec_of + n, d_status = d_prefix + n + 1, d_recs = dn + small_words;
  structure(L, {{"D", L.D, 9 * n}, {"E", L.E, 10 * n}, {"hash", L.hash, 8 * n}, {"rs", L.rs, 16 * n}, {"xy", L.xy, 16 * n}, {"v", L.v, okw}, {"rec", L.rec, 4}, {"ok", L.ok, okw}, {"recovered", L.recovered, 5 * n},
                {"src_of", L.src_of, n}, {"counts", L.counts, nb}, {"bases", L.bases, nb}, {"head", L.head, 4}, {"sp_head", L.sp_head, 4}, {"txhash", L.txhash, 8 * n}, {"froms", L.froms, 5 * n},
                {"rec_froms", L.rec_froms, 5 * n}, {"rec_of", L.rec_of, n}, {"prefix", L.prefix, n + 1}, {"status", L.status, okw}, {"code", L.code, okw}, {"recs", L.recs, 180 * n},
                {"blk_of", L.trie.blk_of, roots ? n : 0}, {"bad", L.trie.bad, n_blocks}, {"node", L.trie.node, roots ? 8 * n : 0}, {"roots", L.trie.roots, 8 * n_blocks}, {"defined", L.trie.defined, up8(n_blocks) / 4}});
  even("recs", L.recs); even("the download's start", L.down);
  eq_upload(L, n, total, n_first); eq_trie(L.trie, tw); eq("the device total", L.end + TXL_SLACK, tw.end + 2); eq("the pinned total", L.pin_bytes, up + 4 * down_words + roots_down);
  eq("the download with every record", 4 * (L.down_end - L.down), 4 * down_words); eq("the small outputs", L.recs - L.down, small_words); eq("the roots' download", 4 * (L.trie.end - L.trie.roots), roots_down);
  eq("D", L.D, D); eq("E", L.E, E); eq("hash", L.hash, hash); eq("rs", L.rs, rs); eq("xy", L.xy, xy); eq("v", L.v, v); eq("rec", L.rec, rec); eq("ok", L.ok, rec + 4); eq("recovered", L.recovered, rec + 4 + okw);
  eq("src_of", L.src_of, src_of); eq("counts", L.counts, counts); eq("bases", L.bases, bases); eq("down", L.down, dn); eq("head", L.head, dn); eq("sp_head", L.sp_head, dn + BH_WORDS); eq("txhash", L.txhash, d_txhash);
  eq("froms", L.froms, d_froms); eq("rec_froms", L.rec_froms, d_rec_froms); eq("rec_of", L.rec_of, d_rec_of); eq("prefix", L.prefix, d_prefix); eq("status", L.status, d_status); eq("code", L.code, d_status + okw);
  eq("recs", L.recs, d_recs);
  const size_t b = 8 * BH_WORDS;
  eq("sp_head in the download", host(L, L.sp_head), 4 * BH_WORDS); eq("txhash in the download", host(L, L.txhash), b); eq("froms in the download", host(L, L.froms), b + 32 * n);
  eq("rec_froms in the download", host(L, L.rec_froms), b + 52 * n); eq("rec_of in the download", host(L, L.rec_of), b + 72 * n); eq("prefix in the download", host(L, L.prefix), b + 76 * n);
  eq("status in the download", host(L, L.status), b + 76 * n + 4 * (n + 1)); eq("code in the download", host(L, L.code), b + 76 * n + 4 * (n + 1) + 4 * okw); eq("recs in the download", host(L, L.recs), 4 * small_words);
  eq("roots behind the download", host(L, L.down_end), 4 * down_words); eq("defined behind the download", host(L, L.down_end) + 4 * (L.trie.defined - L.trie.roots), 4 * down_words + 32 * n_blocks);
}

static void trie_roots(size_t n, size_t total, size_t n_lists, bool want_tx) {
  snprintf(ctx, sizeof ctx, "TrieRootsLayout(%zu, %zu, %zu, %d)", n, total, n_lists, (int)want_tx); const TrieRootsLayout L = trie_roots_layout(n, total, n_lists, want_tx);
  const size_t TD_WORDS = 9, down = 32 * n_lists + up8(n_lists), up = up8(total) + 8 * (n + 1) + up8(4 * (n_lists + 1));
  const size_t okw = (n + 3) / 4, w_walk = want_tx ? (TD_WORDS * n + 16 * n + okw + 1) / 2 * 2 : 0; const WasTrie w = was_trie(up / 4 + w_walk, n, n_lists);
  structure(L, {{"D", L.D, want_tx ? 9 * n : 0}, {"rs", L.rs, want_tx ? 16 * n : 0}, {"v", L.v, want_tx ? okw : 0}, {"blk_of", L.trie.blk_of, n}, {"bad", L.trie.bad, n_lists}, {"node", L.trie.node, 8 * n},
                {"roots", L.trie.roots, 8 * n_lists}, {"defined", L.trie.defined, up8(n_lists) / 4}});   // (with its padding: it comes down to 8 bytes)
  eq_upload(L, n, total, n_lists + 1); eq_trie(L.trie, w); eq("the device total", L.end + TXL_SLACK, w.end + 2); eq("the pinned total", L.pin_bytes, up + down);
  eq("the download", 4 * (L.down_end - L.down), want_tx ? down : 32 * n_lists); eq("down", L.down, w.roots);
  if (want_tx) { eq("D", L.D, up / 4); eq("rs", L.rs, up / 4 + TD_WORDS * n); eq("v", L.v, up / 4 + TD_WORDS * n + 16 * n); }
  eq("roots in the download", host(L, L.trie.roots), 0); eq("defined in the download", host(L, L.trie.defined), 32 * n_lists);
}

static void keccak(size_t n, size_t total) {
  snprintf(ctx, sizeof ctx, "KeccakLayout(%zu, %zu)", n, total); const KeccakLayout L = keccak_layout(n, total); const size_t up = up8(total) + 8 * (n + 1);
  structure(L, {{"out", L.out, 8 * n}});
  eq_upload(L, n, total, 0); eq("the device total", L.end + TXL_SLACK, up / 4 + 8 * n + 2); eq("the pinned total", L.pin_bytes, up + 32 * n); eq("the download", 4 * (L.down_end - L.down), 32 * n);
  eq("out", L.out, up / 4); eq("out in the download", host(L, L.out), 0);
}

// the recovery's output: the head | ok | froms | pubs, as gpu_senders.hip had it (SP_HEAD = 4)
static void senders(size_t n) {
  snprintf(ctx, sizeof ctx, "senders_out(%zu)", n); const size_t okw = (n + 3) / 4;
  for (int pubs = 0; pubs < 2; pubs++) { const SendersOut o = senders_out(n, pubs != 0);
    eq("head", o.head, 0); eq("ok", o.ok, 4); eq("froms", o.froms, 4 + okw); eq("pubs", o.pubs, 4 + okw + 5 * n); eq("the words", o.end, 4 + okw + 5 * n + (pubs ? 16 * n : 0)); }
}

int main() {
  std::vector<size_t> ns, totals; size_t layouts = 0;
  for (size_t n = 0; n <= 17; n++) ns.push_back(n);
  for (size_t n : {63, 64, 65, 127, 128, 129, 255, 256, 257, 32769}) ns.push_back(n);
  for (size_t t = 0; t < 8; t++) { totals.push_back(t); totals.push_back(8 + t); totals.push_back(1000 + t); }   // every residue mod 8: next to nothing, and at a transaction's size
  { Carve c; eq("take", c.take(3), 0); eq("take, aligned", c.take(1, 2), 4); eq("take, nothing", c.take(0, 4), 8); eq("at", c.at, 8); eq("bytes(0)", Carve::bytes(0), 0); eq("bytes(5)", Carve::bytes(5), 2); }
  for (size_t n : ns) {
    senders(n);
    for (size_t total : totals) {
      sender_inputs(n, total); keccak(n, total); layouts += 2;
      for (size_t lists = 0; lists <= 17; lists++) { records(n, total, lists); trie_roots(n, total, lists, false); trie_roots(n, total, lists, true); layouts += 3; }
    }
  }
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("TXS LAYOUT OK: %zu layouts\n", layouts);
  return 0;
}
