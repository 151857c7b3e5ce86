/*
 * edv_measure.h -- measurement entry points of libedv_measure.so, the
 * benchmark/profiling build of the verifier (same sources as libedv.so,
 * compiled with -DEDV_MEASUREMENT_API).  The product library libedv.so does
 * NOT export these: a Node binds include/edv.h only.  bench.py and the
 * profiling tools load libedv_measure.so beside the product library (a
 * second set of device contexts in the same process; device pointers from
 * either library are interchangeable) to time kernels on the kernels' own
 * stream, and the GPU tests use its fault hook.  Every edv.h entry point is
 * exported too, with the product's verdicts.
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
int edv_probe_math(int device, int op, const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint64_t n);

#ifdef __cplusplus
}
#endif
#endif /* EDV_MEASURE_H */
