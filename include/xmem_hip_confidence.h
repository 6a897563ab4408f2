/*
 * xmem_hip_confidence.h - eighth header of libxmem_hip.so: the index mask of a frame's class scores together with a per-pixel margin
 * plane and a per-label record of how sure the prediction was.  xmem2_amd/confidence.py has the definition (`stats_host`) the bytes
 * are held to.
 *
 * The dialect and the conventions are xmem_hip_temporal.h's: functions and #defines only, status codes of xmem_hip.h's xmem_status,
 * device pointers, `stream` a hipStream_t passed as void*, no allocation, no read-back, no host synchronisation: a call is one
 * memset node (the record) and one launch on `stream` and can be captured.  The margin is one float32 subtraction and one product
 * with a power of two, both exact in every rounding mode and under contraction; everything after it is integer.  The only atomics are
 * integer adds into the record, whose sums depend on no order: the same input gives the same bytes on every run.  xmem_hip.h stays at
 * ABI version 5.
 *
 * A MARGIN, not a probability: q says by how much the winner led, in 1/256 of the score range, and nothing about how often it is right.
 */
#ifndef XMEM_HIP_CONFIDENCE_H
#define XMEM_HIP_CONFIDENCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XMEM_CONFIDENCE_MAX_C 255        /* classes (background included): a label fits a byte */
#define XMEM_CONFIDENCE_MAX_TAU 256      /* threshold: q < tau counts as low; 0 counts nothing, 256 everything */
#define XMEM_CONFIDENCE_MAX_PASSES 257   /* of the integer route: 257 * 255 is the largest sum a uint16 holds */
#define XMEM_CONFIDENCE_RECORD 4         /* 64-bit values per label of the record: the four below, in this order */
#define XMEM_CONFIDENCE_AREA 0           /* pixels whose label this is */
#define XMEM_CONFIDENCE_MARGIN_SUM 1     /* the sum of q over them */
#define XMEM_CONFIDENCE_LOW 2            /* those of them with q < tau */
#define XMEM_CONFIDENCE_CONTESTED 3      /* pixels with q < tau whose SECOND label this is */

/* PER PIXEL of prob [C][H][W] (float32, finite): top = the first maximal class (the `v > best` loop of xmem_argmax_u8), second = the
 * first maximal class among the others (none when C == 1), m = prob[top] - prob[second] (prob[top] when C == 1), q = 0 unless m > 0,
 * 255 when m * 256.0f >= 255.0f, else (int)(m * 256.0f).
 *   mask [H][W]  = top (byte for byte xmem_argmax_u8's output); may be null
 *   plane [H][W] = 255 - q: bright means unsure; may be null
 *   record [C][XMEM_CONFIDENCE_RECORD] 64-bit integers (below 2^63: int64 and uint64 read the same), overwritten: the four sums above
 * On non-finite scores the result is unspecified, but nothing is indexed by an unclamped value.
 * XMEM_ERR_BAD_ARG: a null prob or record, a record that is not 8-byte aligned, C outside [1, XMEM_CONFIDENCE_MAX_C], tau outside
 * [0, XMEM_CONFIDENCE_MAX_TAU]; XMEM_ERR_UNSUPPORTED: H or W outside [1, 16384].  Everything is refused before any GPU work. */
int xmem_confidence_f32(const float* prob, int C, int H, int W, int tau, uint8_t* mask, uint8_t* plane, uint64_t* record, void* stream);

/* The same of the test-time ensemble's integer scores: acc [C][H][W] uint16, each the sum of `passes` bytes.  top and second by the
 * same rules, q = min(255, (acc[top] - acc[second]) / passes) in integer division (acc[top] / passes when C == 1).
 * Refusals as above, and XMEM_ERR_BAD_ARG for passes outside [1, XMEM_CONFIDENCE_MAX_PASSES]. */
int xmem_confidence_u16(const uint16_t* acc, int passes, int C, int H, int W, int tau, uint8_t* mask, uint8_t* plane, uint64_t* record,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
