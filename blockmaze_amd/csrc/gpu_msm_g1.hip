// G1 instantiation of the MSM pipeline (kept in its own translation unit: the inlined field arithmetic makes these kernels slow to compile)
#include "msm_impl.hpp"
namespace zk {
struct MsmG1::Impl : MsmImpl<Fq, G1AffineRaw> { using MsmImpl::MsmImpl; };
MsmG1::MsmG1(const G1AffineRaw *p, size_t n, int c, bool fo, bool tables, bool uniform) : impl(new Impl(p, n, c, fo, tables, uniform)) {}
MsmG1::MsmG1(const MsmG1 &peer, bool fo, bool uniform) : impl(new Impl(peer.impl->bases, fo, uniform)) {}
MsmG1::~MsmG1() = default;
std::shared_ptr<WsortBuffers> MsmG1::sort_handle() const { return impl->wfused && impl->ws_leader ? impl->ws : nullptr; }
bool MsmG1::share_sort_with(const std::shared_ptr<WsortBuffers> &leader) {
  if (!impl->wfused || !leader || leader->NB != impl->NB || leader->n != impl->n) return false;
  impl->share_sort(leader);
  return true;
}
void MsmG1::run(const Fe32 *s, const uint32_t *idx) { impl->run(s, idx); }
void MsmG1::run_tagged(const Fe32 *z_all, const WitnessTags &wt, const uint32_t *idx) { impl->run_tagged(z_all, wt, idx); }
bool MsmG1::one_pass_sort() const { return impl->hsort; }
void MsmG1::run_product(const Fe32 *a, const Fe32 *b, const Fe32 *z, bool z_is_table) { impl->run_product(a, b, z, z_is_table); }
void MsmG1::set_label(const char *l) { impl->label = l; }
void MsmG1::set_crowded(bool c) { impl->crowded = c; }
void MsmG1::set_stream(int aux) { impl->stream_id = aux; }
void MsmG1::split_ones_path() { impl->enable_split_ones(); }
host::HG1 MsmG1::result() { impl->finish_sync(); return combine<host::HFq, Fq>(impl->host_sums(), impl->RS, impl->bitsum ? 1 : impl->c); }
size_t MsmG1::size() const { return impl->n; }
const G1AffineRaw *MsmG1::points_dev() const { return impl->points.get(); }
void MsmG1::test_path(uint32_t out[TEST_PATH_WORDS]) const {
  const Impl &m = *impl; const HtailShape ts = htail_shape(m.NB);
  const uint32_t run = m.crowded ? std::max(m.h_run, m.h_run_crowded) : m.h_run;
  const uint32_t marg_block = std::max(1u << ts.hi_bits, (1u << ts.lo_bits) / ts.row_chunks) <= 128 ? 64 : 256;   // (as run_impl launches k_hmarg29)
  const uint32_t v[TEST_PATH_WORDS] = {m.hsort ? 1u : 0u, (uint32_t)m.c, (uint32_t)m.W, m.NB, m.hs.groups, m.hs.low_bits, m.hs.idx_bits, m.hs.region,
      m.h_run, m.h_maxp, m.htail29 ? 1u : 0u, m.last_ll, run, m.any_inf ? 1u : 0u, (uint32_t)m.WB, (uint32_t)m.RS,
      ts.top, ts.lo_bits, ts.hi_bits, ts.row_chunks, marg_block, htail_marg_blocks(ts), htail_marg_count(ts), m.last_flag};
  memcpy(out, v, sizeof v);
}
size_t MsmG1::test_h_state(int what, uint32_t *out, size_t cap_words) {
  Impl &m = *impl;
  if (!m.hsort) throw GpuError("msm: no one-pass sort state on this object");
  HIP_CHECK(hipStreamSynchronize(m.stream()));
  const size_t NB = m.NB, G = m.hs.groups;
  const void *src = nullptr; size_t words = 0;
  switch (what) {
    case 0: src = m.hist(); words = NB; break;
    case 1: src = m.offsets.get(); words = NB; break;
    case 2: src = m.group_n.get(); words = G; break;
    case 3: src = m.entries.get(); words = G * (size_t)m.hs.region; break;
    case 4: if (!m.htail29) throw GpuError("msm: no 29-bit bucket sums on this object"); src = m.hb29.get(); words = NB * (sizeof(Point29Rec) / 4); break;
    default: throw GpuError("msm: unknown state");
  }
  if (words > cap_words) throw GpuError("msm: state buffer too small");
  HIP_CHECK(hipMemcpy(out, src, words * 4, hipMemcpyDeviceToHost));
  return words;
}
void MsmG1::test_wpath(uint32_t out[MSM_WPATH_WORDS]) { impl->test_wpath(out); }
size_t MsmG1::test_w_state(int what, uint32_t *out, size_t cap_words) { return impl->test_w_state(what, out, cap_words); }
}  // namespace zk
