/*
 * edv_measure.h -- measurement entry points of libedv_measure.so, the
 * benchmark/profiling build of the verifier (same sources as libedv.so,
 * compiled with -DEDV_MEASUREMENT_API).  The product library libedv.so does
 * NOT export these: a Node binds include/edv.h only.  bench.py and the
 * profiling tools load libedv_measure.so beside the product library (a
 * second set of device contexts in the same process; device pointers from
 * either library are interchangeable) to time kernels on the kernels' own
 * stream, and the GPU tests use its fault hook, its math probes (the header
 * functions on chosen inputs) and its stage probes (the prep kernel's state
 * read back, the main kernel run on a chosen state, the device tables read
 * back).  Every edv.h entry point is exported too, with the product's
 * verdicts.
 */
#ifndef EDV_MEASURE_H
#define EDV_MEASURE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Launches the verify kernels `iters` times on device-resident inputs between
 * two HIP events recorded on the kernels' own stream; elapsed milliseconds of
 * the whole region.
 */
int edv_time_batch_dev(const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_msgs,
                       const uint64_t *d_msg_off, uint64_t msg_base, uint64_t n, uint8_t *d_accept, int device,
                       int iters, float *ms_out);

/*
 * Average per-launch milliseconds of the two kernels of one batch (n <= chunk),
 * each bracketed by HIP events on the kernels' stream: prep (checks,
 * decompression, SHA-512, [S]B, tables) and main (the joint walk).  The
 * length-bucketing pass runs before each pair, outside the events.
 */
int edv_profile_batch_dev(const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_msgs,
                          const uint64_t *d_msg_off, uint64_t msg_base, uint64_t n, uint8_t *d_accept, int device,
                          int iters, float *ms_prep, float *ms_main);

/*
 * edv_profile_batch_dev with, when flush_bytes > 0, a kernel between prep and
 * main that reads and rewrites a flush_bytes buffer (larger than the 256 MiB
 * Infinity Cache: the prep kernel's tables are evicted before main reads
 * them); ms_flush = that kernel's time.
 */
int edv_profile_batch_dev_flush(const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_msgs,
                                const uint64_t *d_msg_off, uint64_t msg_base, uint64_t n, uint8_t *d_accept,
                                int device, int iters, uint64_t flush_bytes, float *ms_prep, float *ms_flush,
                                float *ms_main);

/*
 * The prep kernel's sides timed apart (n <= chunk, uniform message length):
 * ms[0] hash side alone, ms[1] A side alone, ms[2] R side alone, ms[3] all
 * three in one launch (the product's launch), ms[4] the two point sides in one
 * launch; averages over `iters` launches each, HIP events on the kernels'
 * stream.  The verdicts of such a call are not complete (main is not run).
 */
int edv_profile_prep_sides(const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_msgs,
                           const uint64_t *d_msg_off, uint64_t msg_base, uint64_t n, uint8_t *d_accept, int device,
                           int iters, float ms[5]);

/*
 * Fault hook for the GPU tests of the asynchronous path: the submission that
 * will receive `ticket` on `device` launches no kernels and reports EDV_E_HIP
 * when it completes (edv_wait_async, or a later submission reusing its slot),
 * as a batch whose done event failed would.  ticket < 0 disarms.
 */
int edv_test_fail_async(int device, int64_t ticket);

/*
 * Device math probes: the header functions the kernels are made of
 * (edv_math.h, edv_verify_core.h, edv_quad_math.h), each run unchanged on n
 * independent cases so the GPU tests can compare the DEVICE build of the
 * arithmetic with Python integers on inputs no signature reaches.  Case i is
 * read from in + i * in_stride and its result written to out + i * out_stride
 * (host buffers; strides in bytes, multiples of 4, at least the op's sizes
 * below; words are 32-bit little-endian, limb vectors 10 int32, doubles raw
 * 64-bit patterns).  One kernel launch on the context's stream.
 *
 * One lane per case:
 *   op                      in (bytes)                  out (bytes)
 *   FE_MUL                  f, g limbs (80)             limbs (40)
 *   FE_SQ / SQ2 / SQ_FLOOR  limbs (40)                  limbs (40)
 *   FE_TOBYTES              limbs (40)                  32 bytes
 *   FE_FROMBYTES            32 bytes                    limbs (40)
 *   FE_INVERT_SAFEGCD       limbs (40)                  limbs (40)
 *   FE_POW22523             limbs (40)                  limbs (40)
 *   SC_REDUCE               64 bytes                    32 bytes
 *   HALF_SCALARS            h (32)                      a (32), u (32), neg word (68)
 *   RECODE5                 scalar < 2^253 (32)         recode5 digits (32), digits5_windows word (36)
 *   APPROX_DIV / FDIV_FLOOR a, b doubles (16)           double (8)
 *   EUCLID_DIV              r0, t0, r1, t1 (128)        r0, t0 (64)
 *   GE_FROMBYTES            32 bytes                    words ge_is_canonical, has_small_order,
 *                                                       ge_frombytes_negate, then X Y Z T limbs (172)
 * The batch signer's arithmetic (sign_one, edv_verify_core.h):
 *   SC_MULADD               a, b, c scalars (96)        (a b + c) mod L (32)
 *   RECODE8                 scalar < 2^253 (32)         the 32 packed signed radix-256 digits (32)
 *   SCALARMULT_BASE         k < 2^253 (32)              scalarmult_base's X Y Z T limbs (160), then
 *                                                       ge_p3_tobytes of that point (32): 192.  Walks the
 *                                                       context's own comb table (built on first use, as
 *                                                       edv_sign_batch_dev builds it) through the sign
 *                                                       kernel's GlobalComb view
 *   GE_P3_TOBYTES           X Y Z T limbs (160)         32 bytes
 * One quad (4 consecutive lanes, coordinate q on lane q) per case:
 *   QUAD_SQ_SHIFT           4 x (limbs, sh word) (176)  4 x limbs (160)
 *   QUAD_DBL                4 x limbs (160)             4 x limbs (160)
 *   QUAD_ADD                point 4 x limbs, cached entry 4 x limbs (320)   4 x limbs (160)
 *   QUAD_CACHED             4 x limbs (160)             4 x limbs (160)
 *   QUAD_CACHED_SIGNED      4 x limbs, neg word 0 / -1 (164)                4 x limbs (160)
 */
#define EDV_PROBE_FE_MUL 1
#define EDV_PROBE_FE_SQ 2
#define EDV_PROBE_FE_SQ2 3
#define EDV_PROBE_FE_SQ_FLOOR 4
#define EDV_PROBE_FE_TOBYTES 5
#define EDV_PROBE_FE_FROMBYTES 6
#define EDV_PROBE_FE_INVERT_SAFEGCD 7
#define EDV_PROBE_FE_POW22523 8
#define EDV_PROBE_SC_REDUCE 9
#define EDV_PROBE_HALF_SCALARS 10
#define EDV_PROBE_RECODE5 11
#define EDV_PROBE_APPROX_DIV 12
#define EDV_PROBE_FDIV_FLOOR 13
#define EDV_PROBE_EUCLID_DIV 14
#define EDV_PROBE_GE_FROMBYTES 15
#define EDV_PROBE_QUAD_SQ_SHIFT 16
#define EDV_PROBE_QUAD_DBL 17
#define EDV_PROBE_QUAD_ADD 18
#define EDV_PROBE_QUAD_CACHED 19
#define EDV_PROBE_QUAD_CACHED_SIGNED 20
#define EDV_PROBE_SC_MULADD 21
#define EDV_PROBE_RECODE8 22
#define EDV_PROBE_SCALARMULT_BASE 23
#define EDV_PROBE_GE_P3_TOBYTES 24
int edv_probe_math(int device, int op, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t n);

/*
 * Stage probes: the seam between the batch path's two launches.  The prep
 * kernel hands the main kernel a per-chunk state in HBM (ChunkState,
 * edv_kernels.h); these run the PRODUCT's kernels (the objects libedv.so is
 * linked from; no probe adds device code) on a state the caller reads back or
 * writes, so the GPU tests see every word prep stores and can walk states no
 * SHA-512 output produces.  Host buffers in and out, device buffers that live
 * for the call only, everything on the context's stream, one sync at the end.
 * Bad arguments: EDV_E_ARG, edv_last_error() naming the probe.
 *
 * The state of n slots, as the kernels index it (cap = slot stride of the
 * word-major arrays; 32-bit little-endian words):
 *   array    words / bytes             contents
 *   dig      17 x cap words            dig[w cap + j]: w 0..7 the 64 packed signed 4-bit digits of a,
 *                                      8..15 of |b|, 16: window count | (b < 0) << 8
 *   alive    3 x cap bytes             alive[k cap + j]: side k (0 hash, 1 A, 2 R) passed for slot j
 *   atab     n x 360 words             atab[360 j + 40 e + 10 c + l]: limb l of coordinate c
 *                                      (Y+X, Y-X, Z, 2dT) of entry e = 0..8, e x (-A)
 *   rtab     n x 360 words             the same for e x ([S]B - R)
 *   perm     n words                   slot j holds request perm[j] (length buckets; absent = identity)
 *   accept   n bytes                   by REQUEST: 0 / 1 where a kernel wrote, else EDV_STAGE_SENTINEL
 *
 * edv_probe_prep_state: [bucket kernels,] prep kernel over n <= EDV_STAGE_CAP
 * requests (sigs n x 64, pks n x 32, msgs, msg_off n + 1 absolute offsets into
 * msgs) against table set `set` (EDV_TABLE_SET_COMPACT / _LARGE, built if the GPU
 * has not built it yet), sides side0 .. side0 + nsides - 1 in one launch, or
 * with EDV_STAGE_SPLIT (side0 = 0, nsides = 3) as the split pipeline's two
 * launches, 0 / 1 then 1 / 2.  EDV_STAGE_BUCKETS runs the length-bucket
 * kernels first and returns perm.  Every state array and accept is filled
 * with EDV_STAGE_SENTINEL bytes before the launches, so what comes back shows
 * exactly which bytes the kernels wrote.  The arrays have cap = EDV_STAGE_CAP
 * (reported in *cap); atab, rtab, perm and accept are copied for n slots.
 *
 * edv_probe_main_state: one launch of the main kernel (EDV_STAGE_PRIO: the
 * split pipeline's edv_main_kernel_prio) on the caller's state of n <= cap <=
 * EDV_STAGE_CAP slots; accept (n bytes, sentinel-filled first) comes back.
 * perm may be null; its entries must be below n, and a live slot's window
 * count at most 64 (the domain main_one documents).
 *
 * edv_probe_table: entries (t, j) = tj[2 k], tj[2 k + 1] of a device table as
 * the context's kernels read it, 32 words each (y+x, y-x, 2dxy limbs, 2 words
 * of padding): EDV_TABLE_SET_COMPACT (16 x 32,769: j x 2^(16 t) B),
 * EDV_TABLE_SET_LARGE (12 x 2,097,153: j x 2^(22 t) B; builds the 3 GiB set if
 * this GPU has none) or EDV_TABLE_SET_COMB (the signer's 32 x 129: j x 256^t B).
 * Device-side copies only, no kernel but a missing table's build.
 */
#define EDV_STAGE_CAP 4096
#define EDV_STAGE_SENTINEL 0xA5
#define EDV_STAGE_BUCKETS 1u
#define EDV_STAGE_SPLIT 2u
#define EDV_STAGE_PRIO 4u
#define EDV_TABLE_SET_COMPACT 0
#define EDV_TABLE_SET_LARGE 1
#define EDV_TABLE_SET_COMB 2
int edv_probe_prep_state(int device, const uint8_t *sigs, const uint8_t *pks, const uint8_t *msgs,
                         const uint64_t *msg_off, uint64_t n, int set, int side0, int nsides, uint32_t flags,
                         uint32_t *dig, uint8_t *alive, int32_t *atab, int32_t *rtab, uint32_t *perm,
                         uint8_t *accept, uint64_t *cap);
int edv_probe_main_state(int device, uint64_t n, uint64_t cap, const uint32_t *dig, const uint8_t *alive,
                         const int32_t *atab, const int32_t *rtab, const uint32_t *perm, uint32_t flags,
                         uint8_t *accept);
int edv_probe_table(int device, int set, const int32_t *tj, uint64_t n, int32_t *out);

/*
 * Latency probes: the latency path's kernels (edv_quad.hip: edv_rtl_kernel,
 * sixteen lanes per signature, and edv_quad_kernel, eight) cut at the barrier
 * after their phase 1.  UNLIKE the stage probes above these are NOT the
 * product's kernel objects: a latency kernel keeps its phase-1 results in LDS,
 * so the probe kernels (edv_probe_latency.hip, this library only) instantiate
 * the same header functions the product's kernels are made of
 * (edv_quad_body.h: phase1, rtl_walk, quad_walk) around a copy of the LDS
 * state to or from global memory.
 *
 * kernel: EDV_LAT_RTL (workgroups of 16 slots) or EDV_LAT_QUAD (32 slots).
 * The state of G = ceil(n / slots per workgroup) workgroups of NS slots, every
 * slot of every workgroup, padding slots included (32-bit words):
 *   dig   G x 17 x NS words     dig[(g 17 + w) NS + j]: w 0..7 the packed signed 4-bit digits of a,
 *                               8..15 of |b|, 16: window count | (b < 0) << 8
 *   pt    G x 3 x 40 x NS words pt[((g 3 + k) 40 + w) NS + j]: point k (0: -A, 1: -R, 2: [S]B),
 *                               extended coordinates X | Y | Z | T, 10 limbs each
 *   ok    G x 3 x NS bytes      ok[(g 3 + k) NS + j]: side k (0 hash, 1 A, 2 R) passed
 *
 * edv_probe_latency_phase1: phase1<BITS, NS> over n <= EDV_STAGE_CAP requests
 * against table set `set` (EDV_TABLE_SET_COMPACT / _LARGE), exactly as the
 * product kernel runs it; after the barrier each workgroup copies its L.dig,
 * L.pt and L.ok out.  dig, pt, ok and accept (n bytes: phase 1 writes no
 * verdict) are filled with EDV_STAGE_SENTINEL bytes first.
 *
 * edv_probe_latency_walk: the caller gives the phase-1 state of all `slots`
 * slots (n rounded up to the workgroup's 16 or 32); each workgroup fills its
 * LDS from it, executes the barrier and runs rtl_walk / quad_walk unchanged
 * (the two-walk variant on table scratch sized as the product sizes it).
 * accept (`slots` bytes, sentinel-filled first: the kernels write verdicts
 * for slots below n only) comes back.  flags: none defined, must be 0.  A slot with its three ok bytes set must have a window count of
 * at most 64, the domain the walks (and the right-to-left kernel's counter
 * protocol) are written for.
 *
 * Both: n = 0 returns EDV_OK with nothing launched; bad arguments return
 * EDV_E_ARG, edv_last_error() naming the probe.
 */
#define EDV_LAT_RTL 0
#define EDV_LAT_QUAD 1
int edv_probe_latency_phase1(int device, int kernel, int set, const uint8_t *sigs, const uint8_t *pks,
                             const uint8_t *msgs, const uint64_t *msg_off, uint64_t n, uint32_t *dig, int32_t *pt,
                             uint8_t *ok, uint8_t *accept);
int edv_probe_latency_walk(int device, int kernel, uint64_t n, uint64_t slots, const uint32_t *dig, const int32_t *pt,
                           const uint8_t *ok, uint32_t flags, uint8_t *accept);

#ifdef __cplusplus
}
#endif
#endif /* EDV_MEASURE_H */
