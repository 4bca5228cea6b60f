// extern "C" surface of the sender recovery (include/zk_senders.h, include/zkgpu.h "Senders from signatures"): the arguments are checked here, before anything is
// queued; the device work is gpu_senders.hip's.  Every C++ exception ends at this boundary.
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include "../../include/zkgpu.h"
#include "../../include/zk_senders.h"
#include "gpu.hpp"

extern std::mutex g_gpu_mutex;
extern void zkgpu_set_error(const std::string &s);
namespace zk {
size_t recover_senders(const uint8_t *sighash, const uint8_t *sigs, size_t n, bool homestead, uint8_t *froms, uint8_t *pubs, uint8_t *ok);
void probe_secp_ops(int op, const uint8_t *a, const uint8_t *b, size_t n, uint8_t *out);
void probe_secp_lincomb(const uint8_t *u1, const uint8_t *u2, const uint8_t *px, const uint8_t *py, size_t n, uint8_t *out_xy, uint8_t *out_inf);
void probe_secp_gtable(uint8_t *out);
void senders_counters(uint64_t out[4]);
}
using namespace zk;

static const char *const NO_DEVICE = "no HIP device visible; libzkgpu has no CPU fallback";
// fn runs under the device mutex; ZKGPU_ERR_NO_DEVICE without a device, ZKGPU_ERR_RUNTIME for whatever it throws
template <class Fn> static int guarded_senders(Fn fn) {
  try {
    if (!gpu_available()) { zkgpu_set_error(NO_DEVICE); return ZKGPU_ERR_NO_DEVICE; }
    std::lock_guard<std::mutex> lk(g_gpu_mutex); return fn();
  }
  catch (const std::exception &e) { zkgpu_set_error(e.what()); return ZKGPU_ERR_RUNTIME; }
  catch (...) { zkgpu_set_error("unknown error"); return ZKGPU_ERR_RUNTIME; }
}
// every output as a failure leaves it: nothing is written through a null pointer or for a negative count
static void senders_zero(int n, uint8_t *froms, uint8_t *pubs, unsigned char *ok) {
  if (n <= 0) return;
  if (froms) memset(froms, 0, 20 * (size_t)n);
  if (pubs) memset(pubs, 0, 64 * (size_t)n);
  if (ok) memset(ok, 0, (size_t)n);
}

extern "C" {
int zkgpu_recover_senders(const uint8_t *sighash, const uint8_t *sigs, int n, int homestead, uint8_t *froms, uint8_t *pubs, unsigned char *ok) {
  senders_zero(n, froms, pubs, ok);
  if (n < 0 || (n && (!sighash || !sigs || !froms || !ok))) { zkgpu_set_error("senders: a negative count or a null pointer"); return ZKGPU_ERR_ARG; }   // (before the device is asked for)
  const int rc = guarded_senders([&] {
    return (int)recover_senders(sighash, sigs, (size_t)n, homestead != 0, froms, pubs, ok); });
  if (rc == ZKGPU_ERR_RUNTIME) senders_zero(n, froms, pubs, ok);                                     // a step failed midway: nothing half-written stays
  return rc;
}
int zkRecoverSenders(const uint8_t (*sighash)[32], const uint8_t (*sigs)[65], int n, int homestead, uint8_t (*froms)[20], uint8_t (*pubs)[64], unsigned char *ok) {
  if (n == 0) return 0;
  const int rc = zkgpu_recover_senders((const uint8_t *)sighash, (const uint8_t *)sigs, n, homestead, (uint8_t *)froms, (uint8_t *)pubs, ok);
  if (rc < 0) { fprintf(stderr, "libzkgpu: zkRecoverSenders: %s\n", zkgpu_last_error()); return -1; }
  return rc;
}
int zkgpu_test_secp_ops(int op, const uint8_t *a, const uint8_t *b, size_t n, uint8_t *out) {
  return guarded_senders([&] { probe_secp_ops(op, a, b, n, out); return ZKGPU_OK; });
}
int zkgpu_test_secp_lincomb(const uint8_t *u1, const uint8_t *u2, const uint8_t *px, const uint8_t *py, size_t n, uint8_t *out_xy, uint8_t *out_inf) {
  return guarded_senders([&] { probe_secp_lincomb(u1, u2, px, py, n, out_xy, out_inf); return ZKGPU_OK; });
}
int zkgpu_test_secp_gtable(uint8_t out[15 * 64]) {
  return guarded_senders([&] { if (!out) { zkgpu_set_error("senders: a null pointer"); return ZKGPU_ERR_ARG; } probe_secp_gtable(out); return ZKGPU_OK; });
}
int zkgpu_test_senders_counters(uint64_t out[4]) {
  return guarded_senders([&] { if (!out) { zkgpu_set_error("senders: a null pointer"); return ZKGPU_ERR_ARG; } senders_counters(out); return ZKGPU_OK; });
}
}  // extern "C"
