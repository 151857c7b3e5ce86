// edv_launch.h -- launch wrappers of the kernels in edv_verify.hip and
// edv_prep.hip, for the host runtime (edv_runtime.hip): each launches on
// stream s and returns hipGetLastError().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edv_kernels.h"

namespace edv {

// main walk over va.n slots (blocks = ceil(n / kBlock)); prio: the split
// pipeline's issue-priority variant
hipError_t launch_main_kernel(unsigned blocks, hipStream_t s, const VerifyArgs& va, bool prio);
// length buckets of requests [base, base + n): histogram into ctr[0, kBuckets),
// scatter with cursors ctr[kBuckets, 2 kBuckets) into perm (ctr zeroed by the caller)
hipError_t launch_bucket_kernels(unsigned blocks, hipStream_t s, const uint64_t* off, uint64_t base, uint64_t n,
                                 uint32_t* ctr, uint32_t* perm);
// a shared [S]B table set of shape sh (large or compact), once per GPU:
// sb_words(sh) words at out, then the tables' base points 2^(bits t) B
// (sh.tables ge_p3) as scratch; out holds sb_alloc_bytes(sh) bytes
hipError_t launch_btab_kernel(hipStream_t s, int32_t* out, SbShape sh);
// the batch signer's comb rows (kCombRows x kCombEntries x kBStride words)
hipError_t launch_comb_kernel(hipStream_t s, int32_t* out);
hipError_t launch_sign_kernel(unsigned blocks, hipStream_t s, const uint32_t* seeds, const uint8_t* msgs,
                              const uint64_t* off, uint64_t msg_base, uint64_t n, uint32_t* pks, uint32_t* sigs,
                              const int32_t* comb);
// the latency path (edv_quad.hip): requests base .. base + n - 1 of va in one
// launch, eight lanes per signature (sixteen in launch_rtl_kernel, below);
// qtab: n x kQSigWords words of scratch
hipError_t launch_quad_kernel(hipStream_t s, const VerifyArgs& va, int32_t* qtab);
// the right-to-left latency kernel (no table scratch); at most kRtlMax requests
hipError_t launch_rtl_kernel(hipStream_t s, const VerifyArgs& va);
constexpr uint64_t kRtlMax = 4096;
// accept bytes -> bitmask (ceil(n / 8) bytes)
hipError_t launch_pack_bits_kernel(hipStream_t s, const uint8_t* acc, uint64_t n, uint8_t* bits);
hipError_t launch_sha256_kernel(unsigned blocks, hipStream_t s, const uint8_t* msgs, const uint64_t* off,
                                uint64_t msg_base, uint64_t n, uint32_t* out);
// Merkle-tree extension (edv_merkle.hip; MerklePass: edv_merkle.h): one pass
// over all its tiles (pass 0 hashes the leaves, or with a.in set reads their
// hashes from it; no launch for a pass without items), and the finish (kept entries of the new hashes, root)
struct MerklePass;
hipError_t launch_merkle_pass_kernel(hipStream_t s, const MerklePass& a, const uint8_t* leaves, const uint64_t* off,
                                     uint64_t leaf_base);
hipError_t launch_merkle_finish_kernel(hipStream_t s, uint64_t old_size, uint64_t new_size, const uint32_t* old_hashes,
                                       uint32_t* new_hashes, uint32_t* root);
// per-leaf roots and audit paths (MerkleAppend: edv_merkle.h), after the passes
// on the same stream; no launch for n = 0 or with neither output wanted
struct MerkleAppend;
hipError_t launch_merkle_append_kernel(hipStream_t s, const MerkleAppend& a);
// proof verification (MerkleVerifyInclusion / MerkleVerifyConsistency:
// edv_merkle.h), one lane per proof; a.leaves non-null: the lanes hash their
// leaves, else they read a.leaf_hashes; no launch for n = 0
struct MerkleVerifyInclusion;
struct MerkleVerifyConsistency;
hipError_t launch_merkle_verify_inclusion_kernel(hipStream_t s, const MerkleVerifyInclusion& a);
hipError_t launch_merkle_verify_consistency_kernel(hipStream_t s, const MerkleVerifyConsistency& a);
// proof generation from a stored tree (MerkleProveInclusion /
// MerkleProveConsistency: edv_merkle.h), one lane per proof; no launch for n = 0
struct MerkleProveInclusion;
struct MerkleProveConsistency;
hipError_t launch_merkle_prove_inclusion_kernel(hipStream_t s, const MerkleProveInclusion& a);
hipError_t launch_merkle_prove_consistency_kernel(hipStream_t s, const MerkleProveConsistency& a);
// auditing a stored tree (MerkleAuditNodes / MerkleAuditLeaves: edv_merkle.h),
// one lane per stored entry; summary: two words the launch adds into (bad
// entries, lowest bad position), set to {0, UINT64_MAX} by whoever owns them;
// no launch for an empty slice
struct MerkleAuditNodes;
struct MerkleAuditLeaves;
hipError_t launch_merkle_audit_nodes_kernel(hipStream_t s, const MerkleAuditNodes& a, uint64_t* summary);
hipError_t launch_merkle_audit_leaves_kernel(hipStream_t s, const MerkleAuditLeaves& a, uint64_t* summary);
// catch-up (MerkleCatchup: edv_merkle.h), one lane per reply, after the passes
// on the same stream; no launch for replies = 0
struct MerkleCatchup;
hipError_t launch_merkle_catchup_kernel(hipStream_t s, const MerkleCatchup& a);

}  // namespace edv
