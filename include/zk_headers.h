/* Optional extension of the drop-in surface: a batch of block headers decided from their bytes in one call, on the device.
 *
 * verifyChainBodiesRoots (zk_tx_roots.h) takes want_roots[b] = header.TxHash of block b from the caller.  In the reference the header step comes first: InsertChain
 * and ValidateHeaderChain (core/headerchain.go:207-252) hash every header and check number and parent-hash contiguity, then hand the batch to engine.VerifyHeaders,
 * which for the Clique private net the reference ships is consensus/clique/clique.go:247-369: a header of 17 fields decoded (core/types/block.go:72-90; rlp/decode.go),
 * a dozen standalone field rules (verifyHeader :269-326), the parent link and the timestamp rule (verifyCascadingFields :332-350), and ecrecover(header) (:172-194) —
 * one secp256k1 key recovery and two Keccak-256 hashes per header.  zkHeaders does that for n headers, one lane of the device per header, and returns what the
 * snapshot and verifyChainBodiesRoots need.
 *
 * The fork's types.Header has two fields more than upstream, RTCMT common.Hash and CMT []*common.Hash (block.go:88-89).  Header.Hash() (:105-107) covers all 17;
 * Clique's sigHash was left at the upstream 15 (clique.go:147-169), so the seal covers neither RTCMT nor CMT.
 *
 * Header i is hdrs[off[i] .. off[i+1]): one RLP list as it stands in a block.  off has n + 1 non-decreasing entries.  period and epoch are the engine's
 * (params.CliqueConfig); epoch == 0 means 30000, as clique.New sets it (clique.go:56, :217-219).  now: unix seconds, what verifyHeader reads from the clock (:276).
 * The parent of header 0 as the caller found it (chain.GetHeader(header.ParentHash, number - 1), :343): have_parent (0: there is none), parent_hash,
 * parent_number, parent_time.
 *
 * status[i] is the first rule that applies, in the reference's own order.  Every header is decided against its predecessor in the batch whatever that predecessor's
 * status, as VerifyHeaders passes headers[:i] (:253).
 *   ZK_HDR_MALFORMED  rlp.DecodeBytes(header, &types.Header{}) would return an error (rlp/decode.go; the rules zk_txs.h lists):
 *     - the outer item is a list (:438, :762) whose payload ends exactly at off[i+1] (:142-144, :886), with exactly 17 items (:443-444, :449, :778); size headers are
 *       canonical (:938, :957, :980-985, :891, :1016-1034); a one-byte string below 0x80 must be the byte itself (:662, :423, :726);
 *     - ParentHash, UncleHash, Root, TxHash, ReceiptHash, MixDigest, RTCMT: a string of exactly 32 bytes; Coinbase: 20; Bloom: 256; Nonce: 8 (decodeByteArray
 *       :395-430: a lone byte and a list are refused);
 *     - Difficulty, Number, Time: a string with no leading zero byte (:271-287);
 *     - GasLimit, GasUsed: a string of at most 8 bytes, no leading zero, the byte 0x00 refused (:703-734);
 *     - Extra: any string (:386-393);
 *     - CMT: a list (:323-336) whose every element is a string of exactly 32 bytes (makePtrDecoder :456-478: the field has no "nil" tag; then :395-430);
 *     - this library's own two bounds: a header longer than 2^32 - 1 bytes, and a Number wider than 8 bytes (the reference reads Number.Uint64() everywhere below).
 *     An empty header is malformed.  Every output of a malformed header is zero.
 *   verifyHeader's rules (clique.go:269-319); a checkpoint is number % epoch == 0 (:280), the genesis included:
 *   ZK_HDR_FUTURE                  Time > now (:276); a Time wider than 8 bytes is always future
 *   ZK_HDR_CHECKPOINT_BENEFICIARY  a checkpoint with a Coinbase that is not zero (:281)
 *   ZK_HDR_VOTE                    Nonce neither ff..ff nor 00..00 (:285)
 *   ZK_HDR_CHECKPOINT_VOTE         a checkpoint with Nonce ff..ff (:288)
 *   ZK_HDR_VANITY                  Extra shorter than 32 bytes (:292)
 *   ZK_HDR_SIGNATURE               Extra shorter than 32 + 65 bytes (:295)
 *   ZK_HDR_EXTRA_SIGNERS           no checkpoint, and Extra longer than 97 bytes (:300)
 *   ZK_HDR_CHECKPOINT_SIGNERS      a checkpoint, and (len(Extra) - 97) % 20 != 0 (:303).  The comparison with the snapshot's signers (:357-365) stays with the caller.
 *   ZK_HDR_MIX_DIGEST              MixDigest not zero (:307)
 *   ZK_HDR_UNCLE_HASH              UncleHash not 1dcc4de8dec75d7aab85b567b6ccd41ad312451b948a7413f0a142fd40d49347, the Keccak-256 of c0 (:65, :311)
 *   ZK_HDR_DIFFICULTY              number > 0 and Difficulty neither 1 nor 2 (:315-318)
 *   verifyCascadingFields' rules (:332-350); number 0 ends here with ZK_HDR_OK and a zero signer (:334-336):
 *   ZK_HDR_ANCESTOR                the parent is missing, its Number.Uint64() != number - 1, or its hash differs from ParentHash (:345).  The parent of header i > 0 is
 *                                  header i - 1 of the batch with the hash computed in this call (:340-341); a header behind a malformed one has no parent.  Header 0 has
 *                                  the caller's, and none if have_parent == 0.
 *   ZK_HDR_TIMESTAMP               parent.Time.Uint64() + period > header.Time.Uint64() (:348), in uint64 arithmetic, the wrap included
 *   ZK_HDR_SEAL                    crypto.Ecrecover(sigHash(header), Extra[len - 65:]) fails (:185).  This is not recoverPlain: no ValidateSignatureValues, no low-s rule.
 *                                  The recovery byte is 4 or more (crypto/secp256k1/secp256.go:171-177); R or S is at or above N (libsecp256k1/src/modules/recovery/
 *                                  main_impl.h:48-51) or zero (:96-98); with recovery id 2 or 3, r >= p - N = 0x14551231950b75fc4402da1722fc9baee (:104-107); r is no x of
 *                                  the curve (:110); the key is the point at infinity (:120).
 *   ZK_HDR_SEAL_UNDECIDED          recovery id 2 or 3 with r below that bound (and R, S in range): libsecp256k1 goes on with x = r + N, which the recovery of zk_senders.h
 *                                  does not take.  The caller decides such a header itself.  No random signature lands here: the probability is 2^-128.
 *
 * Which outputs are written when:
 *   - hash: every header that decodes.  The strict decoder makes the re-encoding equal to the input, so it is the Keccak-256 of the bytes as they stand.
 *   - sealhash: every header that decodes and whose Extra has at least 65 bytes, whatever its status (Author() :235-237 reaches sigHash on any such header); zero
 *     otherwise.  It is the Keccak-256 of: a fresh list header; fields 0 - 11 as they stand; a fresh string header and Extra without its last 65 bytes (an empty rest
 *     is 80, a one-byte rest below 0x80 is the byte itself); fields 13 - 14 as they stand.  No RTCMT, no CMT.
 *   - signer: only where status is ZK_HDR_OK and number > 0; zero otherwise.
 *   - coinbase, tx_root, rtcmt, number, time (Time.Uint64(): the low 64 bits), difficulty (Difficulty where it is below 255, otherwise 255), vote (1 for the nonce
 *     ff..ff, otherwise 0), extra_beg and extra_size (the content of Extra, relative to the header's first byte), cmt_beg and cmt_count (the CMT list's payload, 33
 *     bytes an element: a0 and the hash): every header that decodes, whatever its status.
 * tx_root is laid out as verifyChainBodiesRoots takes want_roots.
 *
 * What stays with the caller:
 *   - the snapshot: authorised signers, recents, in-turn difficulty, votes, and the checkpoint list compared with the snapshot's signers.  snapshot.apply and
 *     verifySeal (clique.go:484-502) read only number, signer, coinbase, vote, difficulty and Extra, all of which the call returns;
 *   - misc.VerifyForkHashes (:321), which is one comparison with hash[i]; BadHashes (core/blockchain.go);
 *   - then verifyChainBodiesRoots with want_roots = tx_root.  There is deliberately no combined headers-plus-bodies chain call: the chain call commits state, and it
 *     must not do so for a block whose signer the caller's snapshot has not yet accepted.
 *
 * Not here: ethash or PoW; the snapshot; CMTRoot(header.CMT) against RTCMT, and header.CMT against the sends' ZKCMTS (the reference checks neither on import); uncles
 * and the receipts root; gas-limit rules (this Clique has none); recovery ids 2 and 3 beyond the rule above; any change to the recovery or to the calls of zk_txs.h,
 * zk_bodies.h and zk_tx_roots.h.
 *
 * May be called from any thread; calls are served one at a time.  One upload (the bytes, then off) and one download.  Exported by libzkgpu.so only: a caller that
 * wants it adds -lzkgpu to its link line.
 */
#ifndef ZK_HEADERS_H
#define ZK_HEADERS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { ZK_HDR_OK = 0, ZK_HDR_MALFORMED = 1, ZK_HDR_FUTURE = 2, ZK_HDR_CHECKPOINT_BENEFICIARY = 3, ZK_HDR_VOTE = 4, ZK_HDR_CHECKPOINT_VOTE = 5, ZK_HDR_VANITY = 6,
       ZK_HDR_SIGNATURE = 7, ZK_HDR_EXTRA_SIGNERS = 8, ZK_HDR_CHECKPOINT_SIGNERS = 9, ZK_HDR_MIX_DIGEST = 10, ZK_HDR_UNCLE_HASH = 11, ZK_HDR_DIFFICULTY = 12,
       ZK_HDR_ANCESTOR = 13, ZK_HDR_TIMESTAMP = 14, ZK_HDR_SEAL = 15, ZK_HDR_SEAL_UNDECIDED = 16 };

/* Every output has room for n entries and none may be NULL; parent_hash may be NULL where have_parent == 0.
 * Returns k, the number of leading headers with status ZK_HDR_OK; -1, with every output zeroed, for n < 0, a null pointer with n > 0, a decreasing off, no
 * device, or a failure of any step.  The arguments are checked before the device is asked for.  n = 0 returns 0 and queues nothing. */
int zkHeaders(const uint8_t *hdrs, const uint64_t *off, int n, uint64_t period, uint64_t epoch, uint64_t now, int have_parent, const uint8_t *parent_hash /* 32 bytes */,
              uint64_t parent_number, uint64_t parent_time, uint8_t (*hash)[32], uint8_t (*sealhash)[32], uint8_t (*signer)[20], uint8_t (*coinbase)[20], uint8_t (*tx_root)[32],
              uint8_t (*rtcmt)[32], uint64_t *number, uint64_t *time, uint8_t *difficulty, uint8_t *vote, uint32_t *extra_beg, uint32_t *extra_size, uint32_t *cmt_beg,
              uint32_t *cmt_count, uint8_t *status);

#ifdef __cplusplus
}
#endif
#endif
