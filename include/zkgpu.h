/* zkgpu.h — C-ABI of libzkgpu.so, the MI355X-native engine behind BlockMaze's libzk_{mint,send,deposit,redeem}.so.
 *
 * Two layers:
 *   1. the drop-in layer: the exact cgo symbols of the reference (declared in zk_mint.h / zk_send.h / zk_deposit.h /
 *      zk_redeem.h next to this file), exported by libzkgpu.so and re-exported by the four thin libzk_*.so;
 *   2. this header: the building blocks underneath, exposed so that parity tests and the benchmark can drive each
 *      kernel on its own.  They correspond to the reference's C++ entry points one level below the cgo wrappers:
 *        zkgpu_msm_g1/g2      <- libff::multi_exp / multi_exp_with_mixed_addition
 *                                (libsnark-vnt/depends/libsnark/depends/libff/libff/algebra/scalar_multiplication/multiexp.tcc:403-496)
 *        zkgpu_domain_*       <- libfqfft::evaluation_domain::{FFT,iFFT,cosetFFT,icosetFFT}
 *                                (depends/libfqfft/libfqfft/evaluation_domain/domains/basic_radix2_domain.tcc:48-88, step_radix2_domain.tcc:39-167)
 *        zkgpu_witness_map    <- libsnark::r1cs_to_qap_witness_map (libsnark/reductions/r1cs_to_qap/r1cs_to_qap.tcc:206-334)
 *        zkgpu_prover_*       <- libsnark::r1cs_gg_ppzksnark_prover (zk_proof_systems/ppzksnark/r1cs_gg_ppzksnark/r1cs_gg_ppzksnark.tcc:391-506)
 *                                + the key loading of libsnark-vnt/src/send/sendcgo.cpp:64-81,345
 *
 * Conventions: all pointers are HOST pointers.  A field element is 32 bytes, little-endian, CANONICAL (not Montgomery).
 * G1 affine = x | y (64 bytes), G2 affine = x.c0 | x.c1 | y.c0 | y.c1 (128 bytes); the point at infinity is all zero bytes.
 * Every function returns 0 on success and a negative code on failure; zkgpu_last_error() gives the message.
 * There is NO CPU fallback: without a HIP device every compute entry point fails with ZKGPU_ERR_NO_DEVICE.
 */
#ifndef ZKGPU_H
#define ZKGPU_H
#include <stddef.h>
#include <stdint.h>
#include "zk_records.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ZKGPU_OK 0
#define ZKGPU_ERR_NO_DEVICE (-1)
#define ZKGPU_ERR_ARG (-2)
#define ZKGPU_ERR_RUNTIME (-3)
#define ZKGPU_ERR_UNSATISFIED (-4)

const char *zkgpu_last_error(void);
const char *zkgpu_version(void);
int zkgpu_device_count(void);                       /* number of visible HIP devices (0 on a CPU-only host) */
int zkgpu_device_numa_node(int device);             /* NUMA node of the host socket visible device `device` hangs off (sysfs), -1 unknown: what a rank launcher binds its process to */
int zkgpu_init(void);                               /* create the device context now instead of lazily */

/* ---- device arithmetic probes (parity tests of the __device__ field / curve code) ---------------------------------- */
/* field: 0 = Fr, 1 = Fq.  op: 0 mul, 1 add, 2 sub, 3 inverse(a), 4 square(a), 5 negate(a) */
int zkgpu_test_field_op(int field, int op, const uint8_t *a, const uint8_t *b, uint8_t *out, size_t n);
/* (field ops 6..9 probe the lazy domain of field.cuh: 6 mul, 7 square, 8 sub on operands pushed towards 2p, 9 masked negation; results normalized) */
/* op: 0 mul, 1 square(a), 2 inverse(a) on Fq2 (64-byte elements c0 | c1); 3 square root by key load's fq2_sqrt (keyops.cuh): out = n roots (zero where a is no
   square) followed by n bytes, fq2_sqrt's verdict (1 = a is a square) */
int zkgpu_test_fq2_op(int op, const uint8_t *a, const uint8_t *b, uint8_t *out, size_t n);
/* group: 1 = G1, 2 = G2.  op: 0 general add, 1 double(a), 2 mixed add (b affine), 3 a*k for 32-bit k (k in b's first 4 bytes) */
int zkgpu_test_group_op(int group, int op, const uint8_t *a, const uint8_t *b, uint8_t *out, size_t n);
/* Raw-limb probes of the arithmetic on nine 29-bit limbs (field29_gfx950.inc) and of the point formulas built on it: nothing is converted or normalized on the
   way, an element is its nine uint32 limbs.  field: 0 = Fr29, 1 = Fq29.  a, b, c, d: nine words an element (operands an operation does not take may be null).
   op: 0 mul(a, b), 1 mul2(a, b, c, d), 2 sqr, 3 norm, 4..8 sub<2 / 4 / 6 / 12 / 18>(a, b), 9 cond_neg(a, bit 0 of b's first word), 10 sub_product(a, b),
   11 neg_product, 12 add_raw, 13 barrett, 14 one, 15 unpack (eight words in), 16 pack_words, 17 to_words (eight words and a zero out), 18 fq29_product_is_zero
   (first word out), 19 two lazy butterfly stages of ntt29_lds_pass (Fr29; 45 words out: (a - b) - c | (a + b) + c | either times d | norm(a - the first product)).
   Fr29 has ops 0, 2, 3, 10, 11, 12, 15, 16, 17 and 19; Fq29 all but 19.  out: nine words an element (op 19: 45). */
int zkgpu_test_field29_op(int field, int op, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out, size_t n);
/* op: 0 XYZZ29 madd_head + madd_tail, 1 madd_head + madd_tail_pp (flags: bit 0 P^2 = 0, bit 1 R^2 = 0 mod q), 2 xyzz29_dbl_affine(b), 3 xyzz29_add (flags bit 1: ZZ = 0
   mod q), 4 quad29_add<false>, 5 quad29_add<true>, 6 oct29_add (4 .. 6: flags bit 0 = the sum is the point at infinity; an operand with all-zero ZZ limbs is the
   point at infinity), 7 fq2_29_mul, 8 fq2_29_sqr, 9 XYZZ2_29::madd, 10 a run of 32 mixed additions into one accumulator, the limbs after every one of them.
   Words a point (a | b | out): ops 0, 1: 36 | 19 | 36; 2: - | 19 | 36; 3 .. 5: 36 | 36 | 36; 6: 72 | 72 | 72; 7: 18 | 18 | 18; 8: 18 | - | 18; 9: 72 | 37 | 72; 10: 36 | 32 x 19 | 32 x 36.
   G1: X Y ZZ ZZZ; affine operand: x y sign (bit 0: add the negative).  G2 in op 9: X.c0 X.c1 Y.c0 .. ZZZ.c1, affine x.c0 x.c1 y.c0 y.c1 sign; in op 6 component-major,
   X.c0 Y.c0 ZZ.c0 ZZZ.c0 X.c1 .. ZZZ.c1 (the slots of the eight lanes).  flags: one word a point. */
int zkgpu_test_point29_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out, uint32_t *flags, size_t n);

/* ---- multi-scalar multiplication ------------------------------------------------------------------------------------ */
/* window_bits 0 = choose from n.  filter_ones: bit 0 = treat scalars 0 / 1 specially like multi_exp_with_mixed_addition; bit 1 = the scalars are known to be
   uniform (H query): one-pass sort with fixed slots per bucket, falling back to the two-pass sort if a bucket overflows (results are the same either way). */
int zkgpu_msm_g1(const uint8_t *points, const uint8_t *scalars, size_t n, int window_bits, int filter_ones, uint8_t out[64]);
int zkgpu_msm_g2(const uint8_t *points, const uint8_t *scalars, size_t n, int window_bits, int filter_ones, uint8_t out[128]);

/* resident form for benchmarking: bases stay in HBM, scalars are uploaded once, run() times only the kernels */
typedef struct zkgpu_msm zkgpu_msm;
zkgpu_msm *zkgpu_msm_create(int group, const uint8_t *points, size_t n, int window_bits, int filter_ones);
int zkgpu_msm_set_scalars(zkgpu_msm *h, const uint8_t *scalars, size_t n);
int zkgpu_msm_run(zkgpu_msm *h, uint8_t *out);     /* out: 64 or 128 bytes */
void zkgpu_msm_destroy(zkgpu_msm *h);
/* Test entry points of the uniform-scalar (H query) path of a G1 object; they add no product behaviour.
   zkgpu_test_msm_path: what the object decided when it was created, 24 words: one-pass sort (0 / 1), window bits c, windows W, buckets NB | the sort's shape:
   groups, low bucket bits, index bits, entry slots a group | run length, pieces a bucket (h_maxp), 29-bit tail (0 / 1), lane exponent of the last combine | the
   run length in effect (crowded or not), any key point at infinity, bucket arrays, result slots | the tail's shape: top, lo_bits, hi_bits, row_chunks | workgroup
   size of the marginal kernel, its workgroups, marginal records, the flag word the last one-pass run raised (0: none; bit 0: a region or a bucket's pieces overflowed,
   or a bucket sum was degenerate; bit 1: a degenerate sum in the tail, its result slots from bit 8 on).
   zkgpu_test_msm_set_crowded: the longer accumulation runs a prover takes while other proofs are in flight.
   zkgpu_test_msm_run_product: sum_i (a_i b_i z_i) P_i with the product formed inside the sort kernel (z: one element, or a table of n); canonical operands.
   zkgpu_test_msm_h_state: what the last run left on the device — only meaningful after a run that did not fall back (zkgpu_general_path_repeats): what = 0 entries
   per bucket, 1 where each bucket's entries start, 2 entries per group, 3 the sorted entries (groups x slots; entry = low bucket bits | sign | table index), 4 the
   bucket sums on 29-bit limbs (48 words a bucket: X, Y, ZZ, ZZZ in slots of 12 words, nine limbs each; all-zero ZZ = the point at infinity).  *words = how
   many words were written; an error if cap_words is too small. */
int zkgpu_test_msm_path(zkgpu_msm *h, uint32_t out[24]);
int zkgpu_test_msm_set_crowded(zkgpu_msm *h, int on);
int zkgpu_test_msm_run_product(zkgpu_msm *h, const uint8_t *a, const uint8_t *b, const uint8_t *z, int z_is_table, uint8_t out[64]);
int zkgpu_test_msm_h_state(zkgpu_msm *h, int what, uint32_t *out, size_t cap_words, size_t *words);
/* Test entry points of the witness MSMs' three-launch path (filter_ones bit 0, fixed-base tables, 16 to 128 buckets: windows 5 to 8), G1 and G2 objects alike; they add
   no product behaviour.
   zkgpu_test_msm_wpath: 20 words: on that path (0 / 1), window bits c, windows W, buckets NB | entry slots a bucket (cap), any key point at infinity, result slots,
   leader (1) or follower (0) of its sort | the sort is shared (0 / 1), the flag word the last synchronised fused run raised — read before the repeat on the general path
   (0: none; bit 0: a bucket of the sort overflowed; bit 1: a degenerate sum in the fold or the tail, on G1 with its result slots from bit 8 on, bit 31 = the sum of the
   ones) —, the length of that run's list of ones, the bucket lanes it used (lane_off[NB]) | its slice length T (entries a lane), and the constants the model restates:
   bucket lanes, ones lanes, the smallest slice | bucket arrays, stream (0 main, 1 .. 4 auxiliary), log2(NB), result slots of the tail.
   zkgpu_test_msm_w_state: what the last synchronised fused run left on the device — only meaningful after a run that did not fall back: what = 0 entries per bucket
   (NB words), 1 the first lane of every bucket (NB + 1 words), 2 the list of ones (an entry = 15 g + v - 1: the subset v of the four points 4g .. 4g + 3), 3 every
   bucket's entries end to end, min(fill, cap) words each (an entry = table index i + w n | sign in bit 31).  *words = how many words were written.
   zkgpu_test_msm_share_sort: the follower takes the leader's sort (MSMs over one scalar vector: A and L, B1 and the G2 half of B); returns 1 accepted, 0 refused (either
   side off the path, another size or window), below 0 an error.  The leader is a G1 or a G2 object.
   zkgpu_test_msm_set_stream: -1 the main stream, 0 .. 3 an auxiliary one.
   zkgpu_test_msm_run_pair: the leader's run, then the follower's over the LEADER's scalars (zkgpu_msm_set_scalars on the leader), both enqueued before either result is
   taken.
   zkgpu_test_msm_run_indexed: point i takes the scalar z_all[index[i]] (n_vars canonical elements; index: one word a point of the object).
   zkgpu_test_msm_run_tagged: the sort from an assignment's tags.  z_all: n_vars canonical elements, variable 0 = ONE; tags: a byte a variable (0 zero, 1 one, 2 listed);
   other_vars: the n_other variables tagged 2, ascending; n_other_bound > n_other: the launch is sized by the bound and the length travels in device memory; var_pos
   (or null): n_vars words, a variable's position in the whole index list, 0xffffffff = none; index (or null): one word a point; base: plain query — point i belongs
   to variable base + i; indexed — the first position of this slice.  Every index is checked against n_vars before anything is launched. */
int zkgpu_test_msm_wpath(zkgpu_msm *h, uint32_t out[20]);
int zkgpu_test_msm_w_state(zkgpu_msm *h, int what, uint32_t *out, size_t cap_words, size_t *words);
int zkgpu_test_msm_share_sort(zkgpu_msm *follower, zkgpu_msm *leader);
int zkgpu_test_msm_set_stream(zkgpu_msm *h, int aux);
int zkgpu_test_msm_run_pair(zkgpu_msm *leader, zkgpu_msm *follower, uint8_t *out_leader, uint8_t *out_follower);
int zkgpu_test_msm_run_indexed(zkgpu_msm *h, const uint8_t *z_all, size_t n_vars, const uint32_t *index, uint8_t *out);
int zkgpu_test_msm_run_tagged(zkgpu_msm *h, const uint8_t *z_all, size_t n_vars, const uint8_t *tags, const uint32_t *other_vars, size_t n_other, size_t n_other_bound,
    const uint32_t *var_pos, const uint32_t *index, uint32_t base, uint8_t *out);

/* ---- evaluation domains --------------------------------------------------------------------------------------------- */
size_t zkgpu_domain_size(size_t min_size);          /* m chosen by get_evaluation_domain for this minimum size, 0 if none */
/* op: 0 FFT, 1 iFFT, 2 cosetFFT (g = 5), 3 icosetFFT.  data: m elements, transformed in place */
int zkgpu_domain_transform(size_t min_size, int op, uint8_t *data);

/* ---- R1CS / QAP ------------------------------------------------------------------------------------------------------- */
typedef struct zkgpu_r1cs zkgpu_r1cs;
/* CSR per matrix: rowptr (n_cons+1), col (nnz, 0 = the constant ONE), coeff (nnz x 32 bytes canonical) */
zkgpu_r1cs *zkgpu_r1cs_create(size_t n_inputs, size_t n_vars, size_t n_cons, const uint32_t *const rowptr[3], const uint32_t *const col[3], const uint8_t *const coeff[3]);
void zkgpu_r1cs_destroy(zkgpu_r1cs *cs);
/* z: n_vars elements (without ONE).  h_out: (m+1) elements, m = zkgpu_domain_size(n_cons + n_inputs + 1).  Returns ZKGPU_ERR_UNSATISFIED if z violates a constraint. */
int zkgpu_witness_map(zkgpu_r1cs *cs, const uint8_t *z, uint8_t *h_out);

/* ---- key-side operations (test entries): the host functions of key generation and key load, unchanged, on caller arrays.  Points canonical as everywhere here.
 * zkgpu_test_decompress (group 1 / 2; decompress_g1 / _g2 as groth16_keyio.cpp calls them): xs_mont = n x-coordinates in MONTGOMERY form (32 bytes for G1, c0 | c1 = 64 for
 *   G2), flags: bit 0 = the lsb of canonical y (y.c0 for G2), bit 1 = the point at infinity; points_out: n points.  An x that is on no point is ZKGPU_ERR_RUNTIME, no points.
 * zkgpu_test_fixed_base_mul (fixed_base_mul_g1 / _g2, key generation's window tables): points_out[i] = scalars[i] * base, base affine, scalars canonical.
 * zkgpu_test_h_query_lagrange (Domain::h_query_to_coset_lagrange, ecntt.cuh): h = n_in <= m points (infinity allowed), out = the m points P_j of the domain of
 *   zkgpu_domain_size(min_size) with sum_j v_j P_j = sum_i icosetFFT(v)_i h_i for every v.
 * zkgpu_test_fold_c (Domain::fold_c_into_l on the domain of cs): h_lagrange = m points, L = n_vars - n_inputs points, out = n_vars + 1 points, the L query extended to all
 *   variables minus the C polynomial's share of the H term. */
int zkgpu_test_decompress(int group, const uint8_t *xs_mont, const uint8_t *flags, size_t n, uint8_t *points_out);
int zkgpu_test_fixed_base_mul(int group, const uint8_t *base, const uint8_t *scalars, size_t n, uint8_t *points_out);
int zkgpu_test_h_query_lagrange(size_t min_size, const uint8_t *h, size_t n_in, uint8_t *out);
int zkgpu_test_fold_c(zkgpu_r1cs *cs, const uint8_t *h_lagrange, const uint8_t *L, uint8_t *out);

/* ---- circuits, keys, resident prover, verifier -------------------------------------------------------------------- */
/* kind: 0 mint, 1 send, 2 deposit, 3 redeem (100 / 101 / 102 / 103 = test circuits: libsnark's sha256 two-to-one, Merkle check-read, BlockMaze's less-comparison block, one sha256_CMTA_gadget; 104..106 the CMTS / PRF / CRH blocks; 107 the public-input unpacker over tree_depth bits).  tree_depth only matters for deposit (reference: 8) and kind 107. */
/* writes the circuit's constraint system as an "R1CSBM01" file: magic, u64 n_inputs / n_vars / n_cons, then per matrix u64 nnz, u32 rowptr[n_cons+1], u32 col[nnz], 32-byte coeff[nnz] */
int zkgpu_circuit_export(int kind, int tree_depth, const char *r1cs_path);
/* witness files: u64 n, then n 32-byte canonical values (the full assignment without ONE).  Same arguments as the gen*proof symbols. */
int zkgpu_witness_sha256(const uint8_t left[32], const uint8_t right[32], const char *wit_path);
int zkgpu_witness_lesscmp(uint64_t value_old, uint64_t value_s, const char *wit_path);
int zkgpu_witness_unpacker(int nbits, const uint8_t *bits /* nbits bytes of 0 / 1 */, const char *wit_path);
int zkgpu_witness_hashblock(int which /* 0 CMTS, 1 PRF, 2 CRH: circuit kinds 104..106 of zkgpu_circuit_export */, const uint8_t *bits /* 736 / 512 / 416 bytes of 0 / 1 */, const char *wit_path);
int zkgpu_witness_cmta(const uint8_t *bits /* 576 bytes of 0 / 1: value[64], sn[256], r[256] */, const char *wit_path);
int zkgpu_witness_send(uint64_t value_A, char *r_s, char *sn, char *r, char *cmt_s, char *cmtA, uint64_t value_s, char *pk_recv, uint64_t value_A_new, char *sn_A_new,
                       char *r_A_new, char *cmt_A_new, char *sk, char *pk_sender, const char *wit_path);
int zkgpu_witness_deposit(uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *sns, char *rs, char *cmtB_old, char *cmtB, uint64_t value_s, char *pk,
                          char *sn_A_old, char *cmtS, char *cmtarray, int n, char *sk, int tree_depth, const char *wit_path);
/* kind 101 test circuit: leaf, `depth` siblings (leaf level first, 32 bytes each in hashing byte order) and the leaf position; the root is computed */
int zkgpu_witness_merkle(int depth, const uint8_t leaf[32], const uint8_t *siblings, uint64_t position, const char *wit_path);
int zkgpu_witness_mint_redeem(int redeem, uint64_t value, uint64_t value_old, char *sn_old, char *r_old, char *sn, char *r, char *cmtA_old, char *cmtA, uint64_t value_s, char *sk, const char *wit_path);
/* key generation (r1cs_gg_ppzksnark_generator, r1cs_gg_ppzksnark.tcc:212-388; the *_key executables of libsnark-vnt/src/X/getpvk.cpp).  seed 0 = fresh randomness from the
 * OS; any other seed gives reproducible TEST keys.  Files are written in the reference's key-file format. */
int zkgpu_keygen(int kind, int tree_depth, uint64_t seed, const char *pk_path, const char *vk_path);
int zkgpu_keygen_from_r1cs(const char *r1cs_path, uint64_t seed, const char *pk_path, const char *vk_path);
/* resident prover over a reference-format proving key file */
typedef struct zkgpu_prover zkgpu_prover;
zkgpu_prover *zkgpu_prover_load(const char *pk_path);   /* parses the reference-format key file, or maps its container <pk_path>.gpucache when that is valid; writes the container after a load from text */
int zkgpu_key_container_valid(const char *pk_path);
int zkgpu_test_device_plan(const char *spec, int n_visible, int fallback, int per_device, int *out_devices, int *out_order, int n_order);   /* multi-device pool planning (pure host logic) */
int zkgpu_test_pool_plan(int n_devices, int spill, const int *release_before, int n_calls, int *out_dev);   /* acquire_prover's device choice replayed on the host (capi_zk.cpp) */
int zkgpu_test_scan_blocks(const uint8_t *tags64, const uint64_t *elems64x4, const uint64_t *one4, uint64_t *out10);   /* the hand-over's block classifiers: out[0..2] / [3..5] tag masks scalar / fast, out[6..7] / [8..9] element masks scalar / fast */
int zkgpu_test_equal_columns(const char *r1cs_path, uint32_t *out, size_t cap);   /* host only: groups of variables with identical columns in A, B and C, flattened [size, members ...]; returns the words written / needed */
int zkgpu_test_cgroup_quota(const char *root);   /* the CPU quota the library would respect when sizing its helper pools (host only): CPUs, rounded up, 0 = none */
int zkgpu_test_scan_pool(int callers, int rounds);   /* the hand-over's scan pool driven from several threads at once (host only): rounds served by the pool, -1 on a miscount */
int zkgpu_test_lane_plan(int n_slots, int kinds, int per_kind, int *out_lanes_per_slot);   /* the stream-lane planner with its per-device quota (gpu.hip) */
int zkgpu_test_key_container(const char *path, size_t n_vars, size_t n_cons, size_t m);   /* host-only self-test of the container reader / writer; 0 = passed */     /* 1 if a valid container (matching size / mtime of the key file, checksum) is in place */
/* MSM sharding across GPUs (one process per GPU): a shard holds the contiguous slice rank/world of every query of the key.  prove_partial() runs the whole
 * device pipeline on the resident witness and returns this shard's five partial sums (affine canonical: eA 64 | eB1 64 | eH 64 | eL 64 | eB2 128 = 384 bytes);
 * the records of all ranks are exchanged by the caller (one all-gather) and zkgpu_prover_finish() adds them and assembles the proof on the host. */
zkgpu_prover *zkgpu_prover_load_shard(const char *pk_path, size_t shard_rank, size_t shard_world);
int zkgpu_prover_prove_partial(zkgpu_prover *h, uint8_t out[384]);
int zkgpu_prover_finish(zkgpu_prover *h, const uint8_t *records, size_t n_records, const uint8_t *r, const uint8_t *s, char proof_hex[513]);
void zkgpu_prover_destroy(zkgpu_prover *h);
int zkgpu_prover_info(zkgpu_prover *h, size_t out[3]);          /* n_vars, n_inputs, domain size m */
/* z: n_vars elements; r, s: 32-byte canonical prover randomness or NULL for fresh values.  proof_hex: 512 hex characters + NUL. */
int zkgpu_prover_prove(zkgpu_prover *h, const uint8_t *z, const uint8_t *r, const uint8_t *s, char proof_hex[513]);
/* the two halves of zkgpu_prover_prove: upload the assignment into HBM (returns when it is resident), then prove from there any number of times */
int zkgpu_prover_set_witness(zkgpu_prover *h, const uint8_t *z);
int zkgpu_prover_prove_resident(zkgpu_prover *h, const uint8_t *r, const uint8_t *s, char proof_hex[513]);
/* inputs resident in HBM: keep the assignment handed over last in device memory — the RAW vector, (n_vars + 1) x 32 bytes, nothing derived from it; its slot is
 * returned, a dropped slot is reused — / prove a kept assignment in place: the tags and the list of values other than 0 and 1 (the classification of libsnark's
 * multi_exp_with_mixed_addition, multiexp.tcc:443-496) are derived by a device kernel INSIDE the call; no host buffer, no copy.  What bench.py's `value` times:
 * distinct statements uploaded before the timed region.  drop_stash frees a slot (0xffffffff: all of them); ZKGPU_ERR_* if no assignment was handed over / no such slot. */
int zkgpu_prover_stash_witness(zkgpu_prover *h, uint32_t *slot);
int zkgpu_prover_drop_stash(zkgpu_prover *h, uint32_t slot);
int zkgpu_prover_stash_count(zkgpu_prover *h, uint32_t *count);
/* a kept assignment copied back to the host in the layout zkgpu_prover_set_witness takes (n_vars x 32 bytes, canonical): tests and diagnostics — after a proof has read
 * the slot in place, variables with equal columns hold their folded (equivalent) values */
int zkgpu_prover_read_stash(zkgpu_prover *h, uint32_t slot, uint8_t *z_out);
/* groups of variables whose columns coincide in A, B and C found in this key (their values are folded into one place at the head of every proof: an equivalent assignment,
 * no equal points meeting in an incomplete addition); and, process-wide, how often a fast MSM path raised its flag and the MSM was repeated on the general path */
int zkgpu_prover_equal_column_groups(zkgpu_prover *h, uint32_t *count);
uint64_t zkgpu_general_path_repeats(void);
/* key queries this process loaded WITHOUT their fixed-base tables because the tables did not fit the device's free memory: proofs on such a key are several times slower —
 * a deployment can read the degradation here (and on stderr) instead of guessing it from the proof rate */
uint64_t zkgpu_queries_without_tables(void);
int zkgpu_prover_prove_stashed(zkgpu_prover *h, uint32_t slot, const uint8_t *r, const uint8_t *s, char proof_hex[513]);
/* A second prover object on the same resident key: shares the immutable device tables of `h` (1.8 GB for send), owns its streams and workspaces (about 0.25 GB).
 * Objects may be used from different threads at the same time; their proofs overlap on the device. */
zkgpu_prover *zkgpu_prover_clone(zkgpu_prover *h);
/* n proofs against one resident key in one call (BASELINE.json configs[2]: a batch of independent statements).  zs: n assignments of n_vars 32-byte canonical values each,
 * back to back; rs: n pairs (r, s) of 32-byte canonical values, or NULL for fresh randomness; proofs_hex: n records of 513 bytes.  The proofs are spread over
 * ZK_BATCH_LANES (default 4) prover objects sharing the key's tables, one host thread each, so that the packing of witness i+1 and the latency-bound tails of proof i
 * overlap the kernels of the others.  Every proof is byte-identical to what zkgpu_prover_prove returns for the same (z, r, s).  ZKGPU_ERR_UNSATISFIED if any assignment
 * violates the constraint system (the error text lists which); the other records are still filled. */
int zkgpu_prover_prove_batch(zkgpu_prover *h, const uint8_t *zs, size_t n, const uint8_t *rs, char *proofs_hex);
int zkgpu_prover_timings(zkgpu_prover *h, double out[5]);       /* ms of the last prove(): upload+rows, (unused), device kernels, host finish, total */
/* per-stage device timing with HIP events on the compute stream (for the benchmark's roofline leg).  report: JSON {"stage": {"ms_total": x, "count": n}, ...} */
int zkgpu_profile_enable(int on);
int zkgpu_profile_report(char *buf, size_t cap);
/* 1 = accept, 0 = reject, negative = error.  inputs: n_inputs canonical field elements (the packed public input) */
int zkgpu_verify(const char *vk_path, const char *proof_hex, const uint8_t *inputs, size_t n_inputs);
/* the same decision for n proofs in one GPU launch (kernel K9; r1cs_gg_ppzksnark_verifier_strong_IC, r1cs_gg_ppzksnark.tcc:509-623, one lane per proof).
   proofs_hex: n * 512 characters (no separators); inputs: n * n_inputs canonical field elements of 32 bytes; ok[i] = 1 accept / 0 reject.  Returns ZKGPU_OK or an error */
/* test entry: the GPU verifier's operation schedule interpreted on the host (no device needed); returns 1 accept / 0 reject; stats[8] (optional): rounds, slots, products, linear operations, constants, rounds of products / eight-lane sums / one-lane sums */
int zkgpu_test_verify_schedule(const char *vk_path, const char *proof_hex, const uint8_t *inputs, size_t n_inputs, uint32_t *stats);
/* out[0] = small verification calls (up to 64 proofs) taken by this key's GPU verifier, out[1] = kernel launches made for them: calls that meet — go-ethereum verifies
 * from many goroutines, one proof a call — share a launch */
int zkgpu_verify_counters(const char *vk_path, uint64_t out[2]);
/* test entry: out[0], out[1] as zkgpu_verify_counters; out[2] = launches of the large-batch workgroup-per-proof branch (65 to ZK_VERIFY_WAVE_MAX proofs, default
 * 8,192), out[3] = launches of the lane-per-proof branch (more than ZK_VERIFY_WAVE_MAX proofs) */
int zkgpu_verify_path_counters(const char *vk_path, uint64_t out[4]);
/* test entry (needs a GPU): kernel K9's LDS values after every `every`-th round of its schedule against the host model of the same 29-bit limb arithmetic, on one proof.
 * out[0] = the first round whose values differ or -1, out[1] = the slot, out[2] = the kernel's verdict (1 accept, 0 reject, 2 handed back to the host verifier) */
int zkgpu_test_verify_trace(const char *vk_path, const char *proof_hex, const uint8_t *inputs, size_t n_inputs, uint32_t every, long out[3]);
int zkgpu_verify_batch(const char *vk_path, const char *proofs_hex, const uint8_t *inputs, size_t n_inputs, size_t n, uint8_t *ok);
/* The same verdicts as zkgpu_verify_batch, by ONE randomized pairing-product check over all records of the call (DESIGN.md "Block verification"):
 *   FE(prod_i Miller(A_i, B_i)^{r_i} * Miller(-S_acc, gamma) * Miller(-S_C, delta)) == alpha_g1_beta_g2^{sum r_i}
 * over the records that pass verifyBatch's screen; if it fails (or cannot be formed) every record is decided by the per-proof path.  Probabilistic: a call with a
 * bad record passes the equation with probability at most 1/(2^128 - 1) over the weights.  weights: n x 16 bytes (little-endian r_i, none 0), or NULL for fresh ones from
 * getrandom(2), a draw of 0 drawn again; by_equation (optional): 1 if the equation decided the call.  Calls of fewer than 8,192 records take the per-proof path at once. */
int zkgpu_verify_batch_rlc(const char *vk_path, const char *proofs_hex, const uint8_t *inputs, size_t n_inputs, size_t n, const uint8_t *weights, uint8_t *ok,
                           uint32_t *by_equation);
/* test entries: the equation's left-hand side FE(...) for given weights (gt: 384 bytes, twelve canonical 32-byte little-endian coordinates in libff's order) and
 * 1 if it equals the right-hand side, 0 if not — on the host with pairing_host (no device needed), or through the device path whatever the record count. */
int zkgpu_test_verify_rlc_host(const char *vk_path, const char *proofs_hex, const uint8_t *inputs, size_t n_inputs, size_t n, const uint8_t *weights, uint8_t *gt);
int zkgpu_test_verify_rlc_device(const char *vk_path, const char *proofs_hex, const uint8_t *inputs, size_t n_inputs, size_t n, const uint8_t *weights, uint8_t *gt);
/* process-wide: out[0] = block equations that held, out[1] = equations that failed, out[2] = calls (zkgpu_verify_batch_rlc, verifyBlock) in which no record was
 * decided by an equation */
int zkgpu_verify_rlc_counters(uint64_t out[3]);
/* zkgpu_verify_batch_rlc for records of ONE kind as zk_records.h lays them out (a record of another kind than the first is an argument error): the proofs are
 * parsed and the statements packed on the device (k_ingest_records), by the records' kind; a key whose input count is not the kind's rejects the whole call
 * (strong IC).  weights, ok, by_equation as there. */
int zkgpu_verify_records_rlc(const char *vk_path, const zk_block_record *recs, size_t n, const uint8_t *weights, uint8_t *ok, uint32_t *by_equation);
/* test entries.  zkgpu_test_ingest_records: what the ingest makes of n records of one kind — items_out: n x 256 bytes (A.x A.y | B.x.c0 B.x.c1 B.y.c0 B.y.c1 | C.x C.y,
 * Montgomery; all zero where the 512 characters are not a proof), inputs_out: n x *n_inputs_out canonical field elements (room for 6 a record), parsed_out: n bytes —
 * from the kernel (device = 1) or from the host converter built on proof_from_hex and pack_public_bits (device = 0: needs no device).
 * zkgpu_test_records_rlc: the equation through the device path from records, whatever their count: returns 1 / 0 as zkgpu_test_verify_rlc_device; gt_out: 384 bytes;
 * sums_out: (n_inputs + 1) x 7 words, the device's integers sum r_i and sum r_i x_ij over the records in the equation.
 * zkgpu_test_rlc_sums_host: the same integers by the host loop, for given inputs (n x n_inputs canonical elements), weights and flags (1 = in the equation). */
int zkgpu_test_ingest_records(const zk_block_record *recs, size_t n, int device, uint8_t *items_out, uint8_t *inputs_out, size_t *n_inputs_out, uint8_t *parsed_out);
int zkgpu_test_records_rlc(const char *vk_path, const zk_block_record *recs, size_t n, const uint8_t *weights, uint8_t *gt_out, uint64_t *sums_out);
int zkgpu_test_rlc_sums_host(const uint8_t *inputs, size_t n_inputs, const uint8_t *weights, const uint8_t *flags, size_t n, uint64_t *sums_out);

/* ---- the commitment tree resident in HBM (DESIGN.md "Commitment tree"; the drop-in level is zk_tree.h) -------------------------------------------------
 * An append-only SHA-256 Merkle tree of depth 1..32: node = one compression of left || right from the standard IV without padding, unseen leaves all zero
 * (IncrementalMerkleTree.tcc:179-258, the tree of genRoot at depth 8).  Leaves, siblings and roots are 32 bytes in blob order: the reverse of the 64 hex digits
 * the cgo symbols print.  Entries of one tree are atomic with respect to each other and may be called from any thread. */
typedef struct zkgpu_tree zkgpu_tree;
zkgpu_tree *zkgpu_tree_create(int depth);                                   /* NULL + zkgpu_last_error() on failure */
void zkgpu_tree_destroy(zkgpu_tree *t);
int zkgpu_tree_append(zkgpu_tree *t, const uint8_t *leaves, size_t n);      /* ZKGPU_ERR_ARG if the tree would overflow; nothing changes then */
int zkgpu_tree_size(zkgpu_tree *t, uint64_t *n);
int zkgpu_tree_root(zkgpu_tree *t, uint8_t root[32]);
int zkgpu_tree_path(zkgpu_tree *t, uint64_t index, uint8_t *siblings /* depth x 32, leaf level first */);
int zkgpu_tree_find(zkgpu_tree *t, const uint8_t leaf[32], uint64_t *index); /* the first index holding the blob; ZKGPU_ERR_ARG if absent */
int zkgpu_test_tree_launches(zkgpu_tree *t, uint64_t *launches);            /* test entry: append kernels launched for this tree so far */
/* Past states (DESIGN.md "Past states of the commitment tree"; the drop-in level is zk_tree_states.h).  State m is the tree of the first m leaves, 0 <= m <= size.
 * Each entry checks its arguments before anything runs — ZKGPU_ERR_ARG for a size above the tree's size, an index that is not below its size, a null pointer; nothing
 * is written and nothing changes then — and is at most two kernel launches and one download whatever q is.  q = 0 is a valid call. */
int zkgpu_tree_roots_at(zkgpu_tree *t, const uint64_t *sizes, size_t q, uint8_t *roots /* q x 32 */);   /* sizes in any order, repeats allowed; one launch */
int zkgpu_tree_paths_at(zkgpu_tree *t, uint64_t size, const uint64_t *indices, size_t q, uint8_t *siblings /* q x depth x 32, leaf level first */,
                        uint8_t root[32] /* the root of state `size`; may be NULL */);
int zkgpu_tree_find_at(zkgpu_tree *t, uint64_t size, const uint8_t leaf[32], uint64_t *index);   /* the first of the first `size` leaves holding the blob */
int zkgpu_tree_rewind(zkgpu_tree *t, uint64_t size);                        /* the tree becomes state `size`: the leaves from `size` on are gone */
int zkgpu_test_tree_state_launches(zkgpu_tree *t, uint64_t *launches);      /* test entry: kernels launched by the four entries above and by the proofs at a past size */
/* Anchors (DESIGN.md "A block against the resident tree"; the drop-in level is zk_tree_block.h): match_out[i] = the lowest a with root(sizes[a]) == rts[i], or -1.
 * rts: n x 32 bytes, in blob order or (hash_order != 0) as the bytes of the common.Hash.  One upload, two launches (zkgpu_tree_roots_at's kernel, then the compare,
 * both counted by zkgpu_test_tree_state_launches) and n x 4 bytes back; n = 0 or n_sizes = 0 launches nothing, n_sizes = 0 answers -1 everywhere.  ZKGPU_ERR_ARG with
 * nothing written: a size above the tree's, a null pointer where a count is not 0, n_sizes >= 2^31.  ZKGPU_ERR_NO_DEVICE without a device: there is no host tree. */
int zkgpu_tree_match_roots(zkgpu_tree *t, const uint64_t *sizes, size_t n_sizes, const uint8_t *rts, size_t n, int hash_order, int32_t *match_out);
/* Anchors inside a window (DESIGN.md "A stretch of the chain"; the drop-in level is zk_tree_chain.h): match_out[i] = the lowest a with lo[i] <= a < hi[i] and
 * root(sizes[a]) == rts[i], or -1; lo[i] == hi[i] is an empty window.  Upload, launches, download and counters as zkgpu_tree_match_roots; a workgroup of the compare
 * loads only the roots that the windows of its 256 records cover, so records whose windows lie close together — a segment in block order — cost what their windows
 * hold and not n_sizes.  ZKGPU_ERR_ARG with nothing written: as above, and lo[i] > hi[i] or hi[i] > n_sizes.  ZKGPU_ERR_NO_DEVICE without a device. */
int zkgpu_tree_match_roots_window(zkgpu_tree *t, const uint64_t *sizes, size_t n_sizes, const uint8_t *rts, size_t n, const uint32_t *lo, const uint32_t *hi, int hash_order,
                                  int32_t *match_out);
/* test entry, host only: root (if root != NULL) and, if path != NULL, the path of `index` by notes.cpp's tree_levels */
int zkgpu_test_tree_host(int depth, const uint8_t *leaves, size_t n, uint64_t index, uint8_t root[32], uint8_t *path);

/* ---- the roots of many commitment lists in one call (DESIGN.md "Roots of many lists"; the drop-in level is zk_roots.h) ------------------------------------
 * List i is leaves[first .. first + count) of one shared array of 32-byte leaves; ranges may overlap, coincide or be empty.  roots[i] is the root of the tree
 * above (depth 1..32) over that list alone, an empty list giving the empty root of the depth.  hash_order = 0: leaves and roots in blob order, as the tree entries
 * above; 1: both as the bytes of the common.Hash (zk_records.h), the blob reversed.  ZKGPU_ERR_ARG, with nothing written, for a depth outside 1..32, a range that
 * leaves [0, n_leaves), a count above 2^depth, or a null pointer where a size is not 0.  One upload, a number of kernel launches that depends on the sizes present
 * and not on the number of lists, one download. */
typedef struct { uint64_t first, count; } zkgpu_leaf_range;
int zkgpu_list_roots(int depth, const uint8_t *leaves, size_t n_leaves, const zkgpu_leaf_range *lists, size_t n_lists, int hash_order, uint8_t *roots);
/* test entries: the same roots by notes.cpp's merkle_root, list by list (needs no device); the process-wide number of root-kernel launches so far */
int zkgpu_test_list_roots_host(int depth, const uint8_t *leaves, size_t n_leaves, const zkgpu_leaf_range *lists, size_t n_lists, int hash_order, uint8_t *roots);
int zkgpu_test_list_roots_launches(uint64_t *launches);

/* ---- the set of spent serial numbers resident in HBM (DESIGN.md "Spent serial numbers"; the drop-in level is zk_spent.h) ------------------------------------
 * An append-only log of distinct 20-byte keys in insertion order and an index over it; state m is the first m log entries, 0 <= m <= size.  The index is an
 * open-addressing table of 32-bit slots (a power of two of them, 2^10 at least), linear probing: a slot holds 0 (empty), 0xFFFFFFFF (a tombstone, left by a rewind) or
 * log index + 1.  The home slot of a key: with w0..w4 the key's bytes as five little-endian 32-bit words and seed the set's 64-bit seed (getrandom at creation), in
 * 64-bit arithmetic
 *     h = seed;  for k = 0..4: h = (h ^ w_k) * 0x9E3779B97F4A7C15, h ^= h >> 32;  h = h * 0xD6E8FEB86659FD93, h ^= h >> 32;  home = h & (slots - 1).
 * Live entries + tombstones + the incoming batch stay at or below half of the slots: otherwise the table is first rebuilt at the smallest sufficient size.
 * ZKGPU_ERR_ARG, with nothing written and nothing changed, for a size above the current size, a null pointer, or a log that would reach 2^32 - 2 entries.  Entries of
 * one set are atomic with respect to each other and may be called from any thread.  There is no host set. */
typedef struct zkgpu_snset zkgpu_snset;
zkgpu_snset *zkgpu_snset_create(const uint8_t exempt[20] /* or NULL */);     /* exempt: a key that is never in conflict and never inserted; NULL + zkgpu_last_error() on failure */
void zkgpu_snset_destroy(zkgpu_snset *s);
int zkgpu_snset_size(zkgpu_snset *s, uint64_t *n);
/* The check-then-insert loop of core/state_processor.go:106-163 in record order.  keys: n x 20 bytes; mask: n bytes, or NULL = every record masked in.  Record i is
 * skipped with conflict[i] = 0 if mask[i] == 0 or its key is the exempt key; otherwise conflict[i] = 1 if the key was in the set before the call, else 2 if an earlier
 * record j < i with mask[j] != 0 has the same key, else 0 — and then, if commit != 0, the key is appended to the log (in record order).  size_out (may be NULL): the
 * size after the call.  commit == 0 leaves the set unchanged bit for bit, index included.  One upload, at most one rebuild, three launches, one download. */
int zkgpu_snset_spend(zkgpu_snset *s, const uint8_t *keys, const uint8_t *mask, size_t n, int commit, uint8_t *conflict, uint64_t *size_out);
int zkgpu_snset_query(zkgpu_snset *s, uint64_t size, const uint8_t *keys, size_t q, uint64_t *index /* position in the log if below `size`, else UINT64_MAX = absent */);
int zkgpu_snset_rewind(zkgpu_snset *s, uint64_t size);                       /* the set becomes state `size` */
int zkgpu_snset_read_log(zkgpu_snset *s, uint64_t first, uint64_t count, uint8_t *keys /* count x 20 */);   /* to persist the set, and for tests */
/* test entries: a set with a table of 2^log2_slots slots (4 .. 31; it still grows) and a given seed; the table as it lies in device memory (slots may be NULL: the
 * three numbers alone; otherwise room for *n_slots words as a first call reported them); the process-wide number of kernel launches of all sets so far; and the model
 * the kernels are tested against — stateless, host only, the plain sequential loop: resident = the keys in the set (n_resident x 20), appended receives the keys a
 * commit adds, in order (room for n x 20), n_appended their number */
zkgpu_snset *zkgpu_test_snset_create(int log2_slots, uint64_t seed, const uint8_t exempt[20]);
int zkgpu_test_snset_slots(zkgpu_snset *s, uint32_t *slots, uint64_t *n_slots, uint64_t *seed, uint64_t *tombstones);
int zkgpu_test_snset_launches(uint64_t *launches);
int zkgpu_test_snset_host(const uint8_t *resident, size_t n_resident, const uint8_t exempt[20], const uint8_t *keys, const uint8_t *mask, size_t n, int commit,
                          uint8_t *conflict, uint8_t *appended, size_t *n_appended);
/* The same loop with up to two keys a record (DESIGN.md "Two keys a record"; the drop-in level is zk_spent_pk.h).  keys: n x 2 x 20 bytes, k1 then k2; nkeys[i] = 0
 * (masked out), 1 or 2.  The exempt key applies to k1 only: an exempt k1 is neither checked nor inserted, the record's k2 still is.  In record order: conflict[i] = 1
 * if a key of the record was in the set before the call, or its k2 is the exempt key; else 2 if an earlier ACCEPTED record of this call inserted one of its keys, or
 * k1 == k2; else 0: the record is accepted and, with commit, its keys are appended, k1 before k2.  A rejected record inserts nothing.  With every nkeys[i] <= 1 the
 * codes, the log and the size are those of zkgpu_snset_spend.  ZKGPU_ERR_ARG also for nkeys[i] > 2 and unless size + 2n < 2^32 - 2; the call needs live entries +
 * tombstones + 2n at or below half of the slots.  Four launches a round whatever n is, one round when the batch has no conflict among its own keys; after the round
 * cap (8) the host decides the records still open.  A committing call may leave tombstones where rejected records had claimed slots. */
int zkgpu_snset_spend_pairs(zkgpu_snset *s, const uint8_t *keys, const uint8_t *nkeys, size_t n, int commit, uint8_t *conflict, uint64_t *size_out);
/* test entries: the sequential model of the call above (stateless, host only; appended: room for n x 2 x 20); the round cap of one set (0 = the default); the
 * process-wide numbers of rounds run on the device and of calls the host finished */
int zkgpu_test_snset_host_pairs(const uint8_t *resident, size_t n_resident, const uint8_t exempt[20], const uint8_t *keys, const uint8_t *nkeys, size_t n, int commit,
                                uint8_t *conflict, uint8_t *appended, size_t *n_appended);
int zkgpu_test_snset_round_cap(zkgpu_snset *s, uint32_t rounds);
int zkgpu_test_snset_rounds(uint64_t *rounds, uint64_t *host_finishes);

/* ---- the proof cache (DESIGN.md "Proof cache"; the drop-in level is zk_proof_cache.h) --------------------------------------------------------------------
 * The records whose proof this process has accepted, by key: the first 20 bytes of SHA-256(salt[32] || vktag[32] || record[720]) — salt from getrandom at creation,
 * vktag the SHA-256 of the bytes of the verifying-key file of the record's kind as it was loaded; every byte of the record counts.  Two generations of capacity / 2
 * keys, each a spent set as above without an exempt key: an insert that would take the young one past capacity / 2 drops the old one first, and a call with more
 * than capacity / 2 new records stores the first capacity / 2 in record order.  stats: out = {hits, misses, keys stored, entries held now}; clear empties both
 * generations and leaves the three counters.  Entries of one cache may be called from any thread.  There is no host cache. */
typedef struct zkgpu_proof_cache zkgpu_proof_cache;
zkgpu_proof_cache *zkgpu_proof_cache_create(uint64_t capacity /* entries, 2 or more */);   /* NULL + zkgpu_last_error() on failure */
void zkgpu_proof_cache_destroy(zkgpu_proof_cache *c);
int zkgpu_proof_cache_clear(zkgpu_proof_cache *c);
int zkgpu_proof_cache_stats(zkgpu_proof_cache *c, uint64_t out[4]);
/* test entries: a cache with a given salt; the keys of n records under a salt and the four kinds' tags — out20: n x 20 bytes, 20 zero bytes for a kind above 3 —
 * from the kernel k_record_digest whatever the count (device = 1) or from the host model on the library's own SHA-256 (device = 0: needs no device); the
 * process-wide number of digest-kernel launches so far */
zkgpu_proof_cache *zkgpu_test_proof_cache_create(uint64_t capacity, const uint8_t salt[32]);
int zkgpu_test_record_digests(const uint8_t salt[32], const uint8_t tags[4][32], const zk_block_record *recs, size_t n, int device, uint8_t *out20);
int zkgpu_test_proof_cache_launches(uint64_t *launches);

/* ---- the account table resident in HBM (DESIGN.md "Account table"; the drop-in level is zk_accounts.h) -----------------------------------------------------
 * A map from a 20-byte address to a 32-byte value: an append-only log of entries of 14 words — the address (5), the value (8) and prev (1: log index + 1 of the
 * address's previous entry, or 0) — and an index over it; state m is the first m entries, 0 <= m <= size, and the value of an address at state m is the value of
 * its latest entry below m, or 32 zero bytes.  The index is the spent set's: 32-bit slots, a power of two of them (2^10 at least), linear probing from the home slot
 * of the mix stated above; a slot holds 0, 0xFFFFFFFF (a tombstone, left by a rewind) or log index + 1 of the address's LATEST entry.  Entries + tombstones + the
 * incoming batch stay at or below half of the slots: otherwise the table is first rebuilt from the log at the smallest sufficient size.
 * Every call is one upload and one download whatever n is, with two exceptions: a batch in which one address has more records than the chain cap adds the host's
 * search, one upload and one download; and the first get, rewind or unchained fill after a call that failed midway rebuilds the index first and reads the rebuild's
 * error word back, one more download.  ZKGPU_ERR_ARG, with nothing written and nothing changed, for a size above the current size, a null
 * pointer where a count is not 0, or a log that would reach 2^32 - 2 entries.  ZKGPU_ERR_NO_DEVICE without a device: there is no host table.  Entries of one table
 * are atomic with respect to each other and may be called from any thread. */
typedef struct zkgpu_accts zkgpu_accts;
zkgpu_accts *zkgpu_accts_create(void);                                       /* NULL + zkgpu_last_error() on failure */
void zkgpu_accts_destroy(zkgpu_accts *a);
int zkgpu_accts_size(zkgpu_accts *a, uint64_t *n);
/* addrs[i] (n x 20 bytes) gets values[i] (n x 32), unconditionally and in record order: every record becomes a log entry, and an address that repeats ends at its
 * last record's value.  Three launches. */
int zkgpu_accts_set(zkgpu_accts *a, const uint8_t *addrs, const uint8_t *values, size_t n);
/* out[i] (n x 32) = the value of addrs[i] at state at_size; at_size = -1: the current state.  Read-only, one launch, one lane a query. */
int zkgpu_accts_get(zkgpu_accts *a, const uint8_t *addrs, size_t n, int64_t at_size, uint8_t *out);
/* The OLD slot of each record with kind <= 3 — args[0] for mint, send and redeem, args[2] for deposit — is overwritten with the value of addrs[i], and nothing else
 * of the record's 720 bytes.  chained = 0: the table's current value (one launch).  chained != 0: the NEW slot — args[2] mint / redeem, args[3] send, args[4]
 * deposit — of the closest earlier record of the call with the same address and kind <= 3, else the table's value (three launches).  The table does not change,
 * index included. */
int zkgpu_accts_fill(zkgpu_accts *a, const uint8_t *addrs, zk_block_record *recs, size_t n, int chained);
/* zkgpu_accts_set with the values read from the NEW slots of the records with kind <= 3; the others add nothing */
int zkgpu_accts_commit_chain(zkgpu_accts *a, const uint8_t *addrs, const zk_block_record *recs, size_t n);
/* A stretch of the chain (DESIGN.md "A stretch of the chain with accounts"; the drop-in level is zk_accounts_chain.h).  fill_segment writes what zkgpu_accts_fill
 * with chained = 1 writes, commit_segment appends what zkgpu_accts_commit_chain appends; both find a record's predecessor by the tiled search: records of one
 * address meet inside their tile of 256 records, and an address's list holds one node for each tile it occurs in.  Three launches; a list walk visits at most
 * ceil(m / 256) nodes for the m records with kind <= 3, so with the default chain cap no call of up to 65,536 such records takes the host's search, however many of
 * them one address has. */
int zkgpu_accts_fill_segment(zkgpu_accts *a, const uint8_t *addrs, zk_block_record *recs, size_t n);
int zkgpu_accts_commit_segment(zkgpu_accts *a, const uint8_t *addrs, const zk_block_record *recs, size_t n);
int zkgpu_accts_rewind(zkgpu_accts *a, uint64_t size);                       /* the table becomes state `size`; size 0 empties it */
int zkgpu_accts_read_log(zkgpu_accts *a, uint64_t first, uint64_t count, uint8_t *entries /* count x 56: address, value, prev as a little-endian word */);
/* test entries: a table of 2^log2_slots slots (4 .. 31; it still grows) with a given seed; the index as it lies in device memory (as zkgpu_test_snset_slots); the
 * number of list steps of this table after which a batch's predecessor search goes to the host (0 = the default, 256); the process-wide numbers of kernels
 * launched by all tables and of searches the host finished */
zkgpu_accts *zkgpu_test_accts_create(int log2_slots, uint64_t seed);
int zkgpu_test_accts_slots(zkgpu_accts *a, uint32_t *slots, uint64_t *n_slots, uint64_t *seed, uint64_t *tombstones);
int zkgpu_test_accts_chain_cap(zkgpu_accts *a, uint32_t cap);
int zkgpu_test_accts_launches(uint64_t *launches, uint64_t *host_finishes);

/* ---- senders from signatures (DESIGN.md "Senders from signatures"; the drop-in level is zk_senders.h) --------------------------------------------------------
 * secp256k1 public-key recovery and the Keccak-256 address, one lane a signature, six launches a call: the checks and R's y, the scalars u1 = -m / r and u2 = s / r,
 * 1 R ... 15 R, the walk u1 G + u2 R over 64 windows of 4 bits, the affine key, the address.  1 G ... 15 G lie in a table built once.  One upload of 97 bytes a
 * record and one download of 85 (21 without pubs), through pinned staging; the workspace is kept and grown.
 * zkgpu_recover_senders takes zkRecoverSenders' arguments (as flat arrays) and returns the number of records with ok = 1, or ZKGPU_ERR_ARG (n < 0, a null pointer
 * with n > 0; decided first, before the device is asked for, so it wins over the next), ZKGPU_ERR_NO_DEVICE (there is no host path), ZKGPU_ERR_RUNTIME; every
 * output is zeroed on each of them. */
int zkgpu_recover_senders(const uint8_t *sighash /* n x 32 */, const uint8_t *sigs /* n x 65 */, int n, int homestead, uint8_t *froms /* n x 20 */, uint8_t *pubs /* n x 64, or NULL */,
                          unsigned char *ok);
/* test entries.  Every value is 32 big-endian bytes.
 * secp_ops: out[i] = op(a[i], b[i]), one lane a pair; op: 0 mul, 1 sqr, 2 add, 3 sub, 4 neg, 5 inv, 6 sqrt (a^((p+1)/4)), 7 reduce in the field; 8 mul, 9 inv,
 *   10 reduce mod N.  b may be NULL for the operations of one operand.  mul, sqr and reduce take any 256-bit value; the others canonical values (secp256k1.cuh).
 * secp_lincomb: u1[i] G + u2[i] P[i] through the launches of the recovery (the table of P, the walk, the affine step); u1, u2 below N, P = (px, py) on the curve;
 *   out_xy[i] = X || Y, zero where out_inf[i] = 1.
 * secp_gtable: the resident table as it lies in device memory, k G = X || Y at out + 64 (k - 1), k = 1 .. 15.
 * senders_counters: for the last recovery or lincomb call, how many times a lane of the walk took each exceptional branch of the point addition: out = {equal
 *   operands, opposite operands, the running sum at infinity, result at infinity}. */
int zkgpu_test_secp_ops(int op, const uint8_t *a, const uint8_t *b, size_t n, uint8_t *out);
int zkgpu_test_secp_lincomb(const uint8_t *u1, const uint8_t *u2, const uint8_t *px, const uint8_t *py, size_t n, uint8_t *out_xy, uint8_t *out_inf);
int zkgpu_test_secp_gtable(uint8_t out[15 * 64]);
int zkgpu_test_senders_counters(uint64_t out[4]);

/* ---- sender inputs from raw transactions (the drop-in level is zk_txs.h) ------------------------------------------------------------------------
 * One lane a transaction: k_tx_walk applies the strict RLP decoder's rules to the 26 fields of txdata and leaves a descriptor, R || S and V's byte; k_tx_hash
 * computes the signing hash and the transaction hash (Keccak-256, multi-block sponge over a segmented byte source); zkgpu_tx_senders then runs the recovery's six
 * launches on what lies on the device, and k_tx_finish merges the verdicts.  One upload (txs, then off) and one download, through pinned staging; the workspace
 * is kept and grown.
 * Both take the arguments of zkTxSigningInputs / zkTxSenders (as flat arrays) and return the number of records with status ZK_TX_OK, or ZKGPU_ERR_ARG (n < 0, a
 * null pointer with n > 0, a decreasing off, an unknown signer, chain_id >= 2^62; decided first, before the device is asked for, so it wins over the next),
 * ZKGPU_ERR_NO_DEVICE (there is no host path), ZKGPU_ERR_RUNTIME; every output is zeroed on each of them.  deposit_from and zkgpu_tx_senders' txhash may be NULL. */
int zkgpu_tx_signing_inputs(const uint8_t *txs, const uint64_t *off /* n + 1 */, int n, int signer, uint64_t chain_id, uint8_t *txhash /* n x 32 */, uint8_t *sighash /* n x 32 */,
                            uint8_t *sigs /* n x 65 */, uint8_t *deposit_from /* n x 20, or NULL */, uint8_t *code, uint8_t *status);
int zkgpu_tx_senders(const uint8_t *txs, const uint64_t *off /* n + 1 */, int n, int signer, uint64_t chain_id, uint8_t *txhash /* n x 32, or NULL */, uint8_t *froms /* n x 20 */,
                     uint8_t *code, uint8_t *status);
/* test entry: out[i] = Keccak-256 (padding 0x01 ... 0x80, rate 136) of msgs[off[i] .. off[i+1]), n strings through k_tx_hash's sponge, one lane a string */
int zkgpu_test_keccak256(const uint8_t *msgs, const uint64_t *off, size_t n, uint8_t *out /* n x 32 */);

/* ---- records from the block bodies' bytes (the drop-in level is zk_bodies.h) --------------------------------------------------------------------
 * zkgpu_tx_senders' road with the walk's second descriptor (the positions of the ZK fields; a deposit on HomesteadSigner's road), then k_body_finish (the deposit's
 * key rule, the records of each workgroup), k_body_scan, k_body_scatter (rec_of, the prefix values, rec_froms) and k_body_gather (a wave a record).  One upload, four
 * words that say m, one download with recs[0 .. m).  Takes the arguments of zkTxRecords (as flat arrays; recs: n x 720 bytes) and returns m, or ZKGPU_ERR_ARG (decided
 * first, before the device is asked for), ZKGPU_ERR_NO_DEVICE, ZKGPU_ERR_RUNTIME; every output is zeroed on each of them.  txhash may be NULL. */
int zkgpu_tx_records(const uint8_t *txs, const uint64_t *off /* n + 1 */, int n, int signer, uint64_t chain_id, zk_block_record *recs, uint8_t *rec_froms /* n x 20 */,
                     int32_t *rec_of /* n */, uint8_t *txhash /* n x 32, or NULL */, uint8_t *froms /* n x 20 */, uint8_t *code, uint8_t *status);
/* test entry: k_body_gather reads its source words bytewise (1) or from aligned words and a shift (0, the default) from the next call on: the measurement of §23 */
int zkgpu_test_bodies_gather(int bytewise);

/* ---- trie roots of many lists (the drop-in level is zk_tx_roots.h) ----------------------------------------------------------------------------
 * DeriveSha (core/types/derive_sha.go:32-41) of n_lists DerivableLists in one call: list l holds the values first[l] .. first[l+1] - 1 (n_lists + 1 entries, from 0
 * to n, not decreasing), value i is vals[off[i] .. off[i+1]) and is taken verbatim — no walk, no substitution —, its key is rlp(its index within its list).
 * k_trie_leaf (a lane a value: the one pass over the bytes), k_trie_level once per key nibble depth, deepest first, k_trie_finish (a lane a list).  roots: n_lists
 * x 32, emptyRoot for a list with no value.  One upload, one download.  A value under 32 bytes gives ZKGPU_ERR_ARG: a leaf under 32 bytes would be embedded in its
 * parent (trie/hasher.go:176-178) and the kernels reference every node by hash; transactions that decode (five 32-byte hashes) and receipts (a 256-byte bloom)
 * never are.  Also ZKGPU_ERR_ARG (decided first, before the device is asked for): a negative count, a null pointer with n > 0 or n_lists > 0, a decreasing off, a
 * value of 2^32 - 16 bytes or more (the leaf's three headers fit the sponge's sixteen prefix bytes below that), a first that does not run from 0 to n.  ZKGPU_ERR_NO_DEVICE, ZKGPU_ERR_RUNTIME; roots is zeroed on every error.  n_lists = 0
 * returns ZKGPU_OK and queues nothing. */
int zkgpu_list_trie_roots(const uint8_t *vals, const uint64_t *off /* n + 1 */, int n, const int *first /* n_lists + 1 */, int n_lists, uint8_t *roots /* n_lists x 32 */);
/* zkTxRoots (zk_tx_roots.h) with flat arrays: the walk, then the same three steps with a 0xC0 recipient read as 0x80; defined[b] = 0 and a zero root for a block
 * with a malformed transaction.  Returns the number of defined roots, or ZKGPU_ERR_ARG / ZKGPU_ERR_NO_DEVICE / ZKGPU_ERR_RUNTIME with both outputs zeroed. */
int zkgpu_tx_roots(const uint8_t *txs, const uint64_t *off /* n + 1 */, int n, const int *block_first /* n_blocks + 1 */, int n_blocks, uint8_t *roots /* n_blocks x 32 */,
                   uint8_t *defined /* n_blocks */);

/* ---- headers from their bytes (the drop-in level is zk_headers.h) ------------------------------------------------------------------------------
 * One lane a header: k_hdr_walk applies the strict RLP decoder's rules to the 17 fields of types.Header and Clique's standalone rules, and leaves a descriptor, R || S
 * and the recovery byte from Extra's tail, and the fixed-size outputs; k_hdr_hash computes the seal hash (the upstream 15 fields, Extra less its last 65 bytes) and the
 * header's hash through the sponge over a source of three input ranges; the recovery's six launches run on the seal hashes with homestead = 0; k_hdr_finish decides the
 * link and the timestamp against lane i - 1 and merges the verdicts.  One upload (hdrs, then off) and one download, through pinned staging; the workspace is the one the
 * transaction calls keep.
 * Takes the arguments of zkHeaders (as flat arrays) and returns the number of leading headers with status ZK_HDR_OK, or ZKGPU_ERR_ARG (n < 0, a null pointer with
 * n > 0 — parent_hash only where have_parent != 0 —, a decreasing off; decided first, before the device is asked for), ZKGPU_ERR_NO_DEVICE, ZKGPU_ERR_RUNTIME; every
 * output is zeroed on each of them. */
int zkgpu_headers(const uint8_t *hdrs, const uint64_t *off /* n + 1 */, int n, uint64_t period, uint64_t epoch, uint64_t now, int have_parent, const uint8_t *parent_hash /* 32 */,
                  uint64_t parent_number, uint64_t parent_time, uint8_t *hash /* n x 32 */, uint8_t *sealhash /* n x 32 */, uint8_t *signer /* n x 20 */, uint8_t *coinbase /* n x 20 */,
                  uint8_t *tx_root /* n x 32 */, uint8_t *rtcmt /* n x 32 */, uint64_t *number, uint64_t *time, uint8_t *difficulty, uint8_t *vote, uint32_t *extra_beg,
                  uint32_t *extra_size, uint32_t *cmt_beg, uint32_t *cmt_count, uint8_t *status);

/* ---- block bodies from their bytes (the drop-in level is zk_raw_bodies.h) -----------------------------------------------------------------------
 * The bodies rlp([[tx ...], [uncle ...]]) go up once.  k_split_count, a lane a body, decides the outer list, the two lists in it and every element head of the first
 * with the walk's own head reader; k_split_scan scans the element counts and the payload sizes over the blocks; one synchronise brings n, the packed total and
 * block_first down, and the host lays the workspace out for them; k_split_offsets walks again and writes off, tx_beg and tx_size; k_split_pack copies the payloads of
 * the OK bodies end to end, a lane an aligned 8-byte word, to where every kernel of the transaction calls reads txs.
 * Takes the arguments of zkBodySplit and returns k, the number of leading bodies with status ZK_BODY_OK; ZKGPU_ERR_CAP (zkBodySplit's -2: n > cap; *n_txs,
 * block_first and body_status are valid, tx_beg and tx_size zeroed); or ZKGPU_ERR_ARG (a negative count, a null pointer with n_blocks > 0, a decreasing body_off; decided
 * first, before the device is asked for), ZKGPU_ERR_NO_DEVICE, ZKGPU_ERR_RUNTIME, every output zeroed on each of the three. */
#define ZKGPU_ERR_CAP (-5)
int zkgpu_body_split(const uint8_t *bodies, const uint64_t *body_off /* n_blocks + 1 */, int n_blocks, int cap, uint64_t *tx_beg /* cap */, uint32_t *tx_size /* cap */,
                     int *block_first /* n_blocks + 1 */, uint8_t *body_status /* n_blocks */, int *n_txs);
/* test entry: zkgpu_body_split, and what k_split_offsets and k_split_pack left where the kernels read txs and off: packed, room for body_off[n_blocks] - body_off[0]
 * bytes, of which the packed total is written, and packed_off, cap + 1 values of which n + 1 are written; both zeroed where the call does not return k */
int zkgpu_test_body_split(const uint8_t *bodies, const uint64_t *body_off, int n_blocks, int cap, uint64_t *tx_beg, uint32_t *tx_size, int *block_first, uint8_t *body_status, int *n_txs,
                          uint8_t *packed, uint64_t *packed_off);

#ifdef __cplusplus
}
#endif
#endif
