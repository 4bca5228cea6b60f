// What one product of csrc/secp256k1.cuh compiles to: four kernels that hold one routine each between byte-swapping loads and stores.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iblockmaze_amd/csrc -S --cuda-device-only tools/secp_mul_count.hip -o /tmp/secp_mul_count.s
//   python tools/senders_bench.py --count-isa /tmp/secp_mul_count.s      # VALU lines a kernel, by mnemonic
// profiles/senders.txt quotes the result.  The 24 v_perm_b32 of every kernel and a few moves belong to load_be / store_be, not to the routine.
#include <hip/hip_runtime.h>
#include "secp256k1.cuh"
using namespace zk::secp;
__global__ void k_count_fe_mul(const uint32_t *a, const uint32_t *b, uint32_t *o) { store_be(o + 8 * threadIdx.x, fe_mul(load_be(a + 8 * threadIdx.x), load_be(b + 8 * threadIdx.x))); }
__global__ void k_count_sc_mul(const uint32_t *a, const uint32_t *b, uint32_t *o) { store_be(o + 8 * threadIdx.x, sc_mul(load_be(a + 8 * threadIdx.x), load_be(b + 8 * threadIdx.x))); }
__global__ void k_count_fe_add(const uint32_t *a, const uint32_t *b, uint32_t *o) { store_be(o + 8 * threadIdx.x, fe_add(load_be(a + 8 * threadIdx.x), load_be(b + 8 * threadIdx.x))); }
__global__ void k_count_fe_sub(const uint32_t *a, const uint32_t *b, uint32_t *o) { store_be(o + 8 * threadIdx.x, fe_sub(load_be(a + 8 * threadIdx.x), load_be(b + 8 * threadIdx.x))); }
