// extern "C" surface of the headers decided from their bytes (include/zk_headers.h, include/zkgpu.h "Headers from their bytes"): the arguments are checked here, before
// anything is queued; the device work is gpu_txs.hip's.  Every C++ exception ends at this boundary.
#include <cstdio>
#include <cstring>
#include "txs_host.hpp"
using namespace zk;

// every output as a failure leaves it: nothing is written through a null pointer or for a negative count
static void headers_zero(int n, const HeadersOut &o) {
  if (n <= 0) return;
  const size_t nn = (size_t)n;
  if (o.hash) memset(o.hash, 0, 32 * nn);
  if (o.sealhash) memset(o.sealhash, 0, 32 * nn);
  if (o.signer) memset(o.signer, 0, 20 * nn);
  if (o.coinbase) memset(o.coinbase, 0, 20 * nn);
  if (o.tx_root) memset(o.tx_root, 0, 32 * nn);
  if (o.rtcmt) memset(o.rtcmt, 0, 32 * nn);
  if (o.number) memset(o.number, 0, 8 * nn);
  if (o.time) memset(o.time, 0, 8 * nn);
  if (o.difficulty) memset(o.difficulty, 0, nn);
  if (o.vote) memset(o.vote, 0, nn);
  if (o.extra_beg) memset(o.extra_beg, 0, 4 * nn);
  if (o.extra_size) memset(o.extra_size, 0, 4 * nn);
  if (o.cmt_beg) memset(o.cmt_beg, 0, 4 * nn);
  if (o.cmt_count) memset(o.cmt_count, 0, 4 * nn);
  if (o.status) memset(o.status, 0, nn);
}
// n < 0, a null pointer with n > 0 (parent_hash only where there is a parent), a decreasing off
static bool headers_args_ok(const HeadersIn &in, int n, const HeadersOut &o) {
  const char *why = nullptr;
  const bool outputs = o.hash && o.sealhash && o.signer && o.coinbase && o.tx_root && o.rtcmt && o.number && o.time && o.difficulty && o.vote && o.extra_beg && o.extra_size && o.cmt_beg &&
                       o.cmt_count && o.status;
  if (n < 0) why = ": a negative count";
  else if (n && (!in.hdrs || !in.off || !outputs || (in.have_parent && !in.parent_hash))) why = ": a null pointer";
  else for (int i = 0; i < n && !why; i++) if (in.off[i + 1] < in.off[i]) why = ": offsets decrease";
  if (why) zkgpu_set_error(std::string("headers") + why);
  return !why;
}

extern "C" {
int zkgpu_headers(const uint8_t *hdrs, const uint64_t *off, int n, uint64_t period, uint64_t epoch, uint64_t now, int have_parent, const uint8_t *parent_hash, uint64_t parent_number,
                  uint64_t parent_time, uint8_t *hash, uint8_t *sealhash, uint8_t *signer, uint8_t *coinbase, uint8_t *tx_root, uint8_t *rtcmt, uint64_t *number, uint64_t *time,
                  uint8_t *difficulty, uint8_t *vote, uint32_t *extra_beg, uint32_t *extra_size, uint32_t *cmt_beg, uint32_t *cmt_count, uint8_t *status) {
  const HeadersOut o{hash, sealhash, signer, coinbase, tx_root, rtcmt, number, time, difficulty, vote, extra_beg, extra_size, cmt_beg, cmt_count, status};
  const HeadersIn in{hdrs, off, n > 0 ? (size_t)n : 0, period, epoch, now, have_parent, parent_hash, parent_number, parent_time};
  headers_zero(n, o);
  if (!headers_args_ok(in, n, o)) return ZKGPU_ERR_ARG;
  if (n == 0) return 0;
  const int rc = guarded_device([&] { return (int)headers_decide(in, o); });
  if (rc == ZKGPU_ERR_RUNTIME) headers_zero(n, o);                                                  // a step failed midway: nothing half-written stays
  return rc;
}
int zkHeaders(const uint8_t *hdrs, const uint64_t *off, int n, uint64_t period, uint64_t epoch, uint64_t now, int have_parent, const uint8_t *parent_hash, uint64_t parent_number,
              uint64_t parent_time, uint8_t (*hash)[32], uint8_t (*sealhash)[32], uint8_t (*signer)[20], uint8_t (*coinbase)[20], uint8_t (*tx_root)[32], uint8_t (*rtcmt)[32], uint64_t *number,
              uint64_t *time, uint8_t *difficulty, uint8_t *vote, uint32_t *extra_beg, uint32_t *extra_size, uint32_t *cmt_beg, uint32_t *cmt_count, uint8_t *status) {
  const int rc = zkgpu_headers(hdrs, off, n, period, epoch, now, have_parent, parent_hash, parent_number, parent_time, (uint8_t *)hash, (uint8_t *)sealhash, (uint8_t *)signer, (uint8_t *)coinbase,
                               (uint8_t *)tx_root, (uint8_t *)rtcmt, number, time, difficulty, vote, extra_beg, extra_size, cmt_beg, cmt_count, status);
  if (rc < 0) { fprintf(stderr, "libzkgpu: zkHeaders: %s\n", zkgpu_last_error()); return -1; }
  return rc;
}
}  // extern "C"
