// extern "C" surface of the engine layer (include/zkgpu.h).  Catches every C++ exception at the boundary: the library is
// loaded into a Go process through cgo and must never unwind into it, abort, or install signal handlers.
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/zkgpu.h"
#include "gpu.hpp"
#include "capi_accounts.hpp"

namespace zk {
void probe_field(int field, int op, const uint8_t *a, const uint8_t *b, uint8_t *out, size_t n);
void probe_fq2(int op, const uint8_t *a, const uint8_t *b, uint8_t *out, size_t n);
void probe_group(int group, int op, const uint8_t *a, const uint8_t *b, uint8_t *out, size_t n);
void probe_field29(int field, int op, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out, size_t n);
void probe_point29(int op, const uint32_t *a, const uint32_t *b, uint32_t *out, uint32_t *flags, size_t n);
void probe_fq2_sqrt(const uint8_t *a, uint8_t *out, uint8_t *ok, size_t n);   // gpu_keyops.hip, next to fq2_sqrt
}
using namespace zk;
using namespace zk::host;

static thread_local std::string g_err;
void zkgpu_set_error(const std::string &s) { g_err = s; }
std::mutex g_gpu_mutex;   // one proof pipeline at a time on the device (cgo calls arrive on arbitrary OS threads)

template <class Fn> static int guarded(Fn fn) {
  try { if (!gpu_available()) { g_err = "no HIP device visible; libzkgpu has no CPU fallback"; return ZKGPU_ERR_NO_DEVICE; }
        std::lock_guard<std::mutex> lk(g_gpu_mutex); return fn(); }
  catch (const std::exception &e) { g_err = e.what(); return ZKGPU_ERR_RUNTIME; }
  catch (...) { g_err = "unknown error"; return ZKGPU_ERR_RUNTIME; }
}

// canonical bytes <-> Montgomery records
static void g1_to_raw(const uint8_t *p, G1AffineRaw &o) {
  bool z = true;
  for (int i = 0; i < 64; i++) if (p[i]) z = false;
  if (z) {
    memset(&o, 0, sizeof o);
    return;
  }
  HFq x, y; memcpy(x.l, p, 32); memcpy(y.l, p + 32, 32); x = x.to_mont(); y = y.to_mont(); memcpy(&o.x, x.l, 32); memcpy(&o.y, y.l, 32); }
static void g2_to_raw(const uint8_t *p, G2AffineRaw &o) {
  bool z = true;
  for (int i = 0; i < 128; i++) if (p[i]) z = false;
  if (z) {
    memset(&o, 0, sizeof o);
    return;
  }
  Fe32 *dst = &o.x0; for (int k = 0; k < 4; k++) { HFq v; memcpy(v.l, p + 32 * k, 32); v = v.to_mont(); memcpy(&dst[k], v.l, 32); } }
static void g1_out(const HG1 &p, uint8_t *o) { HFq x, y; p.to_affine(x, y); x = x.from_mont(); y = y.from_mont(); memcpy(o, x.l, 32); memcpy(o + 32, y.l, 32); }
static void g2_out(const HG2 &p, uint8_t *o) {
  HFq2 x, y;
  p.to_affine(x, y);
  HFq v[4] = {x.c0.from_mont(), x.c1.from_mont(), y.c0.from_mont(), y.c1.from_mont()};
  for (int k = 0; k < 4; k++) memcpy(o + 32 * k, v[k].l, 32);
}
// Montgomery records -> canonical bytes (the point at infinity is all zero either way)
static void g1_raw_out(const G1AffineRaw &r, uint8_t *o) { const Fe32 *src = &r.x; for (int k = 0; k < 2; k++) { HFq v; memcpy(v.l, &src[k], 32); v = v.from_mont(); memcpy(o + 32 * k, v.l, 32); } }
static void g2_raw_out(const G2AffineRaw &r, uint8_t *o) { const Fe32 *src = &r.x0; for (int k = 0; k < 4; k++) { HFq v; memcpy(v.l, &src[k], 32); v = v.from_mont(); memcpy(o + 32 * k, v.l, 32); } }
static int auto_window(size_t n) { int lg = 0; while (((size_t)1 << lg) < n) lg++; int c = lg - 2; if (c < 7) c = 7; if (c > 16) c = 16; return c; }

struct zkgpu_msm { int group; size_t n; std::unique_ptr<MsmG1> g1; std::unique_ptr<MsmG2> g2; DevBuf<Fe32> scalars; };

extern "C" {
const char *zkgpu_last_error(void) { return g_err.c_str(); }
const char *zkgpu_version(void) { return "blockmaze_amd 0.1 (gfx950)"; }
int zkgpu_device_count(void) { return gpu_available() ? 1 : 0; }
int zkgpu_device_numa_node(int device) {
  int node = -1;
  guarded([&] { if (gpu_available()) node = gpu_device_numa_node(device); return ZKGPU_OK; });
  return node;
}
int zkgpu_init(void) { return guarded([] { gpu(); return ZKGPU_OK; }); }

int zkgpu_test_field_op(int field, int op, const uint8_t *a, const uint8_t *b, uint8_t *out, size_t n) {
  return guarded([&] { probe_field(field, op, a, b, out, n); return ZKGPU_OK; });
}
int zkgpu_test_fq2_op(int op, const uint8_t *a, const uint8_t *b, uint8_t *out, size_t n) {
  return guarded([&] { if (op == 3) probe_fq2_sqrt(a, out, out + 64 * n, n); else probe_fq2(op, a, b, out, n); return ZKGPU_OK; });
}
int zkgpu_test_group_op(int group, int op, const uint8_t *a, const uint8_t *b, uint8_t *out, size_t n) {
  return guarded([&] { probe_group(group, op, a, b, out, n); return ZKGPU_OK; });
}
int zkgpu_test_field29_op(int field, int op, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out, size_t n) {
  return guarded([&] { probe_field29(field, op, a, b, c, d, out, n); return ZKGPU_OK; });
}
int zkgpu_test_point29_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out, uint32_t *flags, size_t n) {
  return guarded([&] { probe_point29(op, a, b, out, flags, n); return ZKGPU_OK; });
}

zkgpu_msm *zkgpu_msm_create(int group, const uint8_t *points, size_t n, int window_bits, int filter_ones) {
  zkgpu_msm *h = nullptr;
  int rc = guarded([&] { if (group != 1 && group != 2) { g_err = "group must be 1 or 2"; return ZKGPU_ERR_ARG; }
    int c = window_bits ? window_bits : auto_window(n); std::unique_ptr<zkgpu_msm> m(new zkgpu_msm); m->group = group; m->n = n;
    if (group == 1) {
      std::vector<G1AffineRaw> raw(n ? n : 1);
      for (size_t i = 0; i < n; i++) g1_to_raw(points + 64 * i, raw[i]);
      m->g1.reset(new MsmG1(raw.data(), n, c, (filter_ones & 1) != 0, true, (filter_ones & 2) != 0));
    }
    else {
      std::vector<G2AffineRaw> raw(n ? n : 1);
      for (size_t i = 0; i < n; i++) g2_to_raw(points + 128 * i, raw[i]);
      m->g2.reset(new MsmG2(raw.data(), n, c, (filter_ones & 1) != 0, true, (filter_ones & 2) != 0));
    }
    m->scalars = DevBuf<Fe32>(n ? n : 1); h = m.release(); return ZKGPU_OK; });
  return rc == ZKGPU_OK ? h : nullptr;
}
int zkgpu_msm_set_scalars(zkgpu_msm *h, const uint8_t *scalars, size_t n) { return guarded([&] { if (!h || n != h->n) { g_err = "scalar count";
    return ZKGPU_ERR_ARG; }
  if (n) { h->scalars.upload((const Fe32 *)scalars, n); fr_to_mont_dev(h->scalars.get(), n); gpu_sync(); } return ZKGPU_OK; }); }
int zkgpu_msm_run(zkgpu_msm *h, uint8_t *out) { return guarded([&] { if (!h) return ZKGPU_ERR_ARG;
  if (h->group == 1) { h->g1->run(h->scalars.get(), nullptr); g1_out(h->g1->result(), out); } else { h->g2->run(h->scalars.get(), nullptr);
      g2_out(h->g2->result(), out); } return ZKGPU_OK; }); }
void zkgpu_msm_destroy(zkgpu_msm *h) { guarded([&] { delete h; return ZKGPU_OK; }); }
// test entry points of the uniform-scalar (H query) path: which path the object takes, and what a one-pass run left on the device (gpu.hpp: MsmG1::test_path)
int zkgpu_test_msm_path(zkgpu_msm *h, uint32_t out[24]) { return guarded([&] { if (!h || h->group != 1 || !out) { g_err = "a G1 MSM object";
    return ZKGPU_ERR_ARG; }
  static_assert(MsmG1::TEST_PATH_WORDS == 24, "zkgpu.h says 24 words"); h->g1->test_path(out); return ZKGPU_OK; }); }
int zkgpu_test_msm_set_crowded(zkgpu_msm *h, int on) { return guarded([&] { if (!h || h->group != 1) { g_err = "a G1 MSM object"; return ZKGPU_ERR_ARG; }
  h->g1->set_crowded(on != 0); return ZKGPU_OK; }); }
int zkgpu_test_msm_run_product(zkgpu_msm *h, const uint8_t *a, const uint8_t *b, const uint8_t *z, int z_is_table, uint8_t out[64]) {
  return guarded([&] { if (!h || h->group != 1 || !h->n || !a || !b || !z || !out) { g_err = "a non-empty G1 MSM object and three operands"; return ZKGPU_ERR_ARG; }
    // (the operands stay alive until result() has synchronised: a fallback reads them again)
    const size_t n = h->n, nz = z_is_table ? n : 1; DevBuf<Fe32> da(n), db(n), dz(nz);
    da.upload((const Fe32 *)a, n); db.upload((const Fe32 *)b, n); dz.upload((const Fe32 *)z, nz);
    fr_to_mont_dev(da.get(), n); fr_to_mont_dev(db.get(), n); fr_to_mont_dev(dz.get(), nz); gpu_sync();
    h->g1->run_product(da.get(), db.get(), dz.get(), z_is_table != 0); g1_out(h->g1->result(), out); return ZKGPU_OK; }); }
int zkgpu_test_msm_h_state(zkgpu_msm *h, int what, uint32_t *out, size_t cap_words, size_t *words) {
  return guarded([&] { if (!h || h->group != 1 || !out || !words) { g_err = "a G1 MSM object"; return ZKGPU_ERR_ARG; }
    *words = h->g1->test_h_state(what, out, cap_words); return ZKGPU_OK; }); }
// test entry points of the three-launch witness path, both groups (gpu.hpp: MSM_WPATH_WORDS; msm_impl.hpp: test_wpath / test_w_state), and the ways the prover drives it
int zkgpu_test_msm_wpath(zkgpu_msm *h, uint32_t out[20]) { return guarded([&] { if (!h || !out) { g_err = "an MSM object"; return ZKGPU_ERR_ARG; }
  static_assert(MSM_WPATH_WORDS == 20, "zkgpu.h says 20 words"); if (h->group == 1) h->g1->test_wpath(out); else h->g2->test_wpath(out); return ZKGPU_OK; }); }
int zkgpu_test_msm_w_state(zkgpu_msm *h, int what, uint32_t *out, size_t cap_words, size_t *words) {
  return guarded([&] { if (!h || !out || !words) { g_err = "an MSM object"; return ZKGPU_ERR_ARG; }
    *words = h->group == 1 ? h->g1->test_w_state(what, out, cap_words) : h->g2->test_w_state(what, out, cap_words); return ZKGPU_OK; }); }
int zkgpu_test_msm_share_sort(zkgpu_msm *follower, zkgpu_msm *leader) {   // 1 accepted, 0 refused
  return guarded([&] { if (!follower || !leader || follower == leader) { g_err = "two MSM objects"; return ZKGPU_ERR_ARG; }
    const std::shared_ptr<WsortBuffers> hd = leader->group == 1 ? leader->g1->sort_handle() : leader->g2->sort_handle();
    return (follower->group == 1 ? follower->g1->share_sort_with(hd) : follower->g2->share_sort_with(hd)) ? 1 : 0; }); }
int zkgpu_test_msm_set_stream(zkgpu_msm *h, int aux) { return guarded([&] { if (!h || aux < -1 || aux > 3) { g_err = "an MSM object and a stream in -1 .. 3"; return ZKGPU_ERR_ARG; }
  if (h->group == 1) h->g1->set_stream(aux); else h->g2->set_stream(aux); return ZKGPU_OK; }); }
static void msm_enqueue(zkgpu_msm *h, const Fe32 *z, const uint32_t *idx) { if (h->group == 1) h->g1->run(z, idx); else h->g2->run(z, idx); }
static void msm_take(zkgpu_msm *h, uint8_t *out) { if (h->group == 1) g1_out(h->g1->result(), out); else g2_out(h->g2->result(), out); }
int zkgpu_test_msm_run_pair(zkgpu_msm *leader, zkgpu_msm *follower, uint8_t *out_leader, uint8_t *out_follower) {
  return guarded([&] { if (!leader || !follower || leader == follower || !leader->n || leader->n != follower->n || !out_leader || !out_follower) {
      g_err = "two non-empty MSM objects of one size"; return ZKGPU_ERR_ARG; }
    // both in flight before either result is taken, the follower over the leader's scalars, as in a proof
    msm_enqueue(leader, leader->scalars.get(), nullptr); msm_enqueue(follower, leader->scalars.get(), nullptr);
    msm_take(leader, out_leader); msm_take(follower, out_follower); return ZKGPU_OK; }); }
// canonical elements -> Montgomery form on the device (synchronised)
static void upload_fr(DevBuf<Fe32> &d, const uint8_t *z, size_t n) { d.upload((const Fe32 *)z, n); fr_to_mont_dev(d.get(), n); gpu_sync(); }
int zkgpu_test_msm_run_indexed(zkgpu_msm *h, const uint8_t *z_all, size_t n_vars, const uint32_t *index, uint8_t *out) {
  return guarded([&] { if (!h || !h->n || !z_all || !n_vars || !index || !out) { g_err = "a non-empty MSM object, scalars and an index"; return ZKGPU_ERR_ARG; }
    for (size_t i = 0; i < h->n; i++) if (index[i] >= n_vars) { g_err = "an index beyond the scalars"; return ZKGPU_ERR_ARG; }
    DevBuf<Fe32> dz(n_vars); DevBuf<uint32_t> di(h->n); upload_fr(dz, z_all, n_vars); di.upload(index, h->n);
    msm_enqueue(h, dz.get(), di.get()); msm_take(h, out); return ZKGPU_OK; }); }
int zkgpu_test_msm_run_tagged(zkgpu_msm *h, const uint8_t *z_all, size_t n_vars, const uint8_t *tags, const uint32_t *other_vars, size_t n_other, size_t n_other_bound,
    const uint32_t *var_pos, const uint32_t *index, uint32_t base, uint8_t *out) {
  return guarded([&] { if (!h || !h->n || !z_all || !n_vars || !tags || (n_other && !other_vars) || !out) { g_err = "a non-empty MSM object, an assignment and its tags"; return ZKGPU_ERR_ARG; }
    // everything the kernels index with is checked here: they trust the prover's arrays
    if (n_other_bound < n_other || n_other_bound >= (1u << 30) || n_vars >= (1ull << 31)) { g_err = "the list's bound"; return ZKGPU_ERR_ARG; }
    for (size_t j = 0; j < n_other; j++) if (other_vars[j] >= n_vars) { g_err = "a listed variable beyond the assignment"; return ZKGPU_ERR_ARG; }
    if (index) { for (size_t i = 0; i < h->n; i++) if (index[i] >= n_vars) { g_err = "an index beyond the assignment"; return ZKGPU_ERR_ARG; } }
    else if ((size_t)base + h->n > n_vars) { g_err = "the slice leaves the assignment"; return ZKGPU_ERR_ARG; }
    DevBuf<Fe32> dz(n_vars); DevBuf<uint8_t> dt(n_vars); DevBuf<uint32_t> dl(n_other_bound ? n_other_bound : 1), dn(1), dp(var_pos ? n_vars : 1), di(index ? h->n : 1);
    upload_fr(dz, z_all, n_vars); dt.upload(tags, n_vars); dl.zero(); if (n_other) dl.upload(other_vars, n_other);
    const uint32_t len = (uint32_t)n_other; dn.upload(&len, 1); if (var_pos) dp.upload(var_pos, n_vars); if (index) di.upload(index, h->n);
    gpu_sync();
    WitnessTags wt; wt.tags = dt.get(); wt.other_vars = dl.get(); wt.n_other = (uint32_t)n_other_bound; wt.n_other_dev = n_other_bound > n_other ? dn.get() : nullptr;
    wt.var_pos = var_pos ? dp.get() : nullptr; wt.base = base;
    if (h->group == 1) h->g1->run_tagged(dz.get(), wt, index ? di.get() : nullptr); else h->g2->run_tagged(dz.get(), wt, index ? di.get() : nullptr);
    msm_take(h, out); return ZKGPU_OK; }); }
static int msm_oneshot(int group,const uint8_t *points, const uint8_t *scalars, size_t n, int c, int fo, uint8_t *out) {
  zkgpu_msm *h = zkgpu_msm_create(group, points, n, c, fo);
  if (!h) return ZKGPU_ERR_RUNTIME;
  int rc = zkgpu_msm_set_scalars(h, scalars, n);
  if (rc == ZKGPU_OK) rc = zkgpu_msm_run(h, out);
  zkgpu_msm_destroy(h);
  return rc;
}
int zkgpu_msm_g1(const uint8_t *points, const uint8_t *scalars, size_t n, int c, int fo, uint8_t out[64]) {
  return msm_oneshot(1, points, scalars, n, c, fo, out);
}
int zkgpu_msm_g2(const uint8_t *points, const uint8_t *scalars, size_t n, int c, int fo, uint8_t out[128]) {
  return msm_oneshot(2, points, scalars, n, c, fo, out);
}

size_t zkgpu_domain_size(size_t min_size) {   // pure host logic: get_evaluation_domain.tcc:33-52 restricted to basic / step radix-2
  if (min_size <= 1) return 0; size_t lg = 0; while (((size_t)1 << lg) < min_size) lg++; if (min_size == ((size_t)1 << lg)) return lg <= 28 ? min_size : 0;
  size_t big = (size_t)1 << (lg - 1), small = min_size - big, rs = 1;
  while (rs < small) rs <<= 1;
  size_t m = (small == rs) ? min_size : big + rs;
  return lg <= 28 ? m : 0;
}
int zkgpu_domain_transform(size_t min_size, int op, uint8_t *data) { return guarded([&] { Domain d(min_size); size_t m = d.m(); DevBuf<Fe32> buf(m);
    buf.upload((const Fe32 *)data, m); fr_to_mont_dev(buf.get(), m);
  switch (op) {
    case 0: d.fft(buf.get(), 1, m);
    break;
    case 1: d.ifft(buf.get(), 1, m);
    break;
    case 2: d.coset_fft(buf.get(), 1, m);
    break;
    case 3: d.icoset_fft(buf.get(), 1, m);
    break;
    default: g_err = "op";
    return ZKGPU_ERR_ARG;
  }
  fr_from_mont_dev(buf.get(), m); buf.download((Fe32 *)data, m); return ZKGPU_OK; }); }

struct zkgpu_r1cs { R1csHost host; std::unique_ptr<R1csDev> dev; std::unique_ptr<Domain> dom; };
zkgpu_r1cs *zkgpu_r1cs_create(size_t n_inputs, size_t n_vars, size_t n_cons, const uint32_t *const rowptr[3], const uint32_t *const col[3],
    const uint8_t *const coeff[3]) {
  zkgpu_r1cs *out = nullptr;
  guarded([&] { std::unique_ptr<zkgpu_r1cs> h(new zkgpu_r1cs); h->host.n_inputs = n_inputs; h->host.n_vars = n_vars; h->host.n_cons = n_cons;
    for (int m = 0; m < 3; m++) {
      size_t nnz = rowptr[m][n_cons];
      h->host.rowptr[m].assign(rowptr[m], rowptr[m] + n_cons + 1);
      h->host.col[m].assign(col[m], col[m] + nnz);
      h->host.coeff[m].resize(nnz);
      if (nnz) memcpy(h->host.coeff[m].data(), coeff[m], 32 * nnz);
    }
    h->dev.reset(new R1csDev(h->host)); h->dom.reset(new Domain(n_cons + n_inputs + 1)); out = h.release(); return ZKGPU_OK; });
  return out;
}
void zkgpu_r1cs_destroy(zkgpu_r1cs *cs) { guarded([&] { delete cs; return ZKGPU_OK; }); }
int zkgpu_witness_map(zkgpu_r1cs *cs, const uint8_t *z, uint8_t *h_out) { return guarded([&] { if (!cs) return ZKGPU_ERR_ARG;
  size_t m = cs->dom->m(), nv = cs->host.n_vars; std::vector<Fe32> zz(nv + 1); memset(&zz[0], 0, 32); zz[0].l[0] = 1; if (nv) memcpy(&zz[1], z, 32 * nv);
  DevBuf<Fe32> zd(nv + 1), abc(3 * m); zd.upload(zz.data(), nv + 1); fr_to_mont_dev(zd.get(), nv + 1);
  cs->dev->eval(zd.get(), abc.get(), m);
  if (!cs->dev->satisfied(abc.get(), m)) {
    g_err = "assignment does not satisfy the constraint system";
    return ZKGPU_ERR_UNSATISFIED;
  }
  // r1cs_to_qap.tcc:239-322 with d1 = d2 = d3 = 0
  cs->dom->ifft(abc.get(), 3, m);
  cs->dom->coset_fft(abc.get(), 3, m);
  cs->dom->qap_pointwise(abc.get(), abc.get() + m, abc.get() + 2 * m);
  cs->dom->icoset_fft(abc.get(), 1, m);
  fr_from_mont_dev(abc.get(), m); abc.download((Fe32 *)h_out, m); memset(h_out + 32 * m, 0, 32); return ZKGPU_OK; }); }

// ---- test entries of the key-side operations: the host functions key generation and key load call, unchanged, on caller arrays ----
int zkgpu_test_decompress(int group, const uint8_t *xs_mont, const uint8_t *flags, size_t n, uint8_t *points_out) {
  return guarded([&] { if (group != 1 && group != 2) { g_err = "group must be 1 or 2"; return ZKGPU_ERR_ARG; }
    if (group == 1) { std::vector<G1AffineRaw> p(n ? n : 1); decompress_g1((const Fe32 *)xs_mont, flags, n, p.data()); for (size_t i = 0; i < n; i++) g1_raw_out(p[i], points_out + 64 * i); }
    else { std::vector<G2AffineRaw> p(n ? n : 1); decompress_g2((const Fe32 *)xs_mont, flags, n, p.data()); for (size_t i = 0; i < n; i++) g2_raw_out(p[i], points_out + 128 * i); }
    return ZKGPU_OK; });
}
int zkgpu_test_fixed_base_mul(int group, const uint8_t *base, const uint8_t *scalars, size_t n, uint8_t *points_out) {
  return guarded([&] { if (group != 1 && group != 2) { g_err = "group must be 1 or 2"; return ZKGPU_ERR_ARG; }
    if (group == 1) { G1AffineRaw b; g1_to_raw(base, b); HFq x, y; memcpy(x.l, &b.x, 32); memcpy(y.l, &b.y, 32);
      std::vector<G1AffineRaw> p(n ? n : 1); fixed_base_mul_g1(HG1::from_affine(x, y), (const Fe32 *)scalars, n, p.data()); for (size_t i = 0; i < n; i++) g1_raw_out(p[i], points_out + 64 * i); }
    else { G2AffineRaw b; g2_to_raw(base, b); HFq2 x, y; memcpy(x.c0.l, &b.x0, 32); memcpy(x.c1.l, &b.x1, 32); memcpy(y.c0.l, &b.y0, 32); memcpy(y.c1.l, &b.y1, 32);
      std::vector<G2AffineRaw> p(n ? n : 1); fixed_base_mul_g2(HG2::from_affine(x, y), (const Fe32 *)scalars, n, p.data()); for (size_t i = 0; i < n; i++) g2_raw_out(p[i], points_out + 128 * i); }
    return ZKGPU_OK; });
}
int zkgpu_test_h_query_lagrange(size_t min_size, const uint8_t *h, size_t n_in, uint8_t *out) {
  return guarded([&] { Domain d(min_size); const size_t m = d.m(); if (n_in > m) { g_err = "n_in exceeds the domain"; return ZKGPU_ERR_ARG; }
    std::vector<G1AffineRaw> in(n_in ? n_in : 1), res(m); for (size_t i = 0; i < n_in; i++) g1_to_raw(h + 64 * i, in[i]);
    d.h_query_to_coset_lagrange(in.data(), n_in, res.data()); for (size_t j = 0; j < m; j++) g1_raw_out(res[j], out + 64 * j); return ZKGPU_OK; });
}
int zkgpu_test_fold_c(zkgpu_r1cs *cs, const uint8_t *h_lagrange, const uint8_t *L, uint8_t *out) {
  return guarded([&] { if (!cs) return ZKGPU_ERR_ARG; const size_t m = cs->dom->m(), nl = cs->host.n_vars - cs->host.n_inputs, n_all = cs->host.n_vars + 1;
    std::vector<G1AffineRaw> p(m), l(nl ? nl : 1), res(n_all); for (size_t j = 0; j < m; j++) g1_to_raw(h_lagrange + 64 * j, p[j]); for (size_t i = 0; i < nl; i++) g1_to_raw(L + 64 * i, l[i]);
    cs->dom->fold_c_into_l(p.data(), cs->host, l.data(), res.data()); for (size_t v = 0; v < n_all; v++) g1_raw_out(res[v], out + 64 * v); return ZKGPU_OK; });
}
}  // extern "C"

// ---- the account table resident in HBM (DESIGN.md "Account table"; include/zkgpu.h) -----------------------------------------------------------------------------
template <class Fn> static int guarded_accts(zkgpu_accts *a, Fn fn) {
  try {
    if (!gpu_available()) { g_err = "no HIP device visible; libzkgpu has no CPU fallback"; return ZKGPU_ERR_NO_DEVICE; }
    if (!a) { g_err = "no account table"; return ZKGPU_ERR_ARG; }
    return fn();
  }
  catch (const std::exception &e) { g_err = e.what(); return ZKGPU_ERR_RUNTIME; }
  catch (...) { g_err = "unknown error"; return ZKGPU_ERR_RUNTIME; }
}
static zkgpu_accts *accts_create(int log2_slots, const uint64_t *seed) {
  zkgpu_accts *a = nullptr;
  try {
    if (!gpu_available()) { g_err = "no HIP device visible; libzkgpu has no CPU fallback"; return nullptr; }
    a = new zkgpu_accts(log2_slots, seed);
  }
  catch (const std::exception &e) { g_err = e.what(); } catch (...) { g_err = "unknown error"; }
  return a;
}
extern "C" {
zkgpu_accts *zkgpu_accts_create(void) { return accts_create(0, nullptr); }
zkgpu_accts *zkgpu_test_accts_create(int log2_slots, uint64_t seed) {
  if (log2_slots < 4 || log2_slots > 31) { g_err = "account table: a table has 2^4 to 2^31 slots"; return nullptr; }
  return accts_create(log2_slots, &seed); }
void zkgpu_accts_destroy(zkgpu_accts *a) { try { delete a; } catch (...) {} }
int zkgpu_accts_size(zkgpu_accts *a, uint64_t *n) { return guarded_accts(a, [&] { if (!n) return ZKGPU_ERR_ARG; *n = a->a.size(); return ZKGPU_OK; }); }
int zkgpu_accts_set(zkgpu_accts *a, const uint8_t *addrs, const uint8_t *values, size_t n) { return guarded_accts(a, [&] {
  if (!a->a.set(addrs, values, n, nullptr)) { g_err = "account table: a null pointer, or the log would reach 2^32 - 2 entries"; return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_accts_get(zkgpu_accts *a, const uint8_t *addrs, size_t n, int64_t at_size, uint8_t *out) { return guarded_accts(a, [&] {
  if (!a->a.get(addrs, n, at_size, out)) { g_err = "account table: size " + std::to_string(at_size) + " is above the table's size, or a null pointer"; return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_accts_fill(zkgpu_accts *a, const uint8_t *addrs, zk_block_record *recs, size_t n, int chained) { return guarded_accts(a, [&] {
  if (!a->a.fill(addrs, (uint8_t *)recs, n, chained != 0)) { g_err = "account table: a null pointer, or more records than the log has room for"; return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_accts_commit_chain(zkgpu_accts *a, const uint8_t *addrs, const zk_block_record *recs, size_t n) { return guarded_accts(a, [&] {
  if (!a->a.commit_chain(addrs, (const uint8_t *)recs, n, nullptr)) { g_err = "account table: a null pointer, or the log would reach 2^32 - 2 entries"; return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_accts_fill_segment(zkgpu_accts *a, const uint8_t *addrs, zk_block_record *recs, size_t n) { return guarded_accts(a, [&] {
  if (!a->a.fill_segment(addrs, (uint8_t *)recs, n)) { g_err = "account table: a null pointer, or more records than the log has room for"; return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_accts_commit_segment(zkgpu_accts *a, const uint8_t *addrs, const zk_block_record *recs, size_t n) { return guarded_accts(a, [&] {
  if (!a->a.commit_segment(addrs, (const uint8_t *)recs, n, nullptr)) { g_err = "account table: a null pointer, or the log would reach 2^32 - 2 entries"; return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_accts_rewind(zkgpu_accts *a, uint64_t size) { return guarded_accts(a, [&] {
  if (!a->a.rewind(size)) { g_err = "account table: cannot rewind to " + std::to_string(size) + " entries, the table holds fewer"; return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_accts_read_log(zkgpu_accts *a, uint64_t first, uint64_t count, uint8_t *entries) { return guarded_accts(a, [&] {
  if (!a->a.read_log(first, count, entries)) { g_err = "account table: the range leaves the log, or a null pointer"; return ZKGPU_ERR_ARG; }
  return ZKGPU_OK; }); }
int zkgpu_test_accts_slots(zkgpu_accts *a, uint32_t *slots, uint64_t *n_slots, uint64_t *seed, uint64_t *tombstones) { return guarded_accts(a, [&] {
  if (!n_slots || !seed || !tombstones) return ZKGPU_ERR_ARG;
  std::vector<uint32_t> t; uint64_t sd = 0, tb = 0; a->a.table(t, sd, tb);
  if (slots) { if (*n_slots != t.size()) { g_err = "account table: the table has " + std::to_string(t.size()) + " slots"; return ZKGPU_ERR_ARG; } memcpy(slots, t.data(), 4 * t.size()); }
  *n_slots = t.size(); *seed = sd; *tombstones = tb; return ZKGPU_OK; }); }
int zkgpu_test_accts_chain_cap(zkgpu_accts *a, uint32_t cap) { return guarded_accts(a, [&] { a->a.set_chain_cap(cap); return ZKGPU_OK; }); }
int zkgpu_test_accts_launches(uint64_t *launches, uint64_t *host_finishes) {
  if (!launches || !host_finishes) return ZKGPU_ERR_ARG;
  if (!gpu_available()) { g_err = "no HIP device visible; libzkgpu has no CPU fallback"; return ZKGPU_ERR_NO_DEVICE; }
  AccountTable::launches(*launches, *host_finishes); return ZKGPU_OK; }
}  // extern "C"
