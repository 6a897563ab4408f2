/*
 * xmem_hip_temporal.h - sixth header of libxmem_hip.so: a sliding majority vote along the time axis of uint8 index masks.
 * xmem2_amd/temporal.py has the definition (`mode_host`) the bytes are held to.
 *
 * The dialect and the conventions are xmem_hip_matte.h's: functions and #defines only, status codes of xmem_hip.h's xmem_status,
 * device pointers, `stream` a hipStream_t passed as void*, no allocation, no read-back, no host synchronisation: a call is one
 * memset node (the counters) and one launch on `stream` and can be captured.  Integer arithmetic; the only atomics are the integer
 * adds into `changed`, whose sum depends on no order: the same input gives the same bytes on every run.  xmem_hip.h stays at ABI
 * version 5.
 *
 * NOTHING exists outside the video: a window is clipped at frame 0 and at frame T - 1 and is never padded.
 */
#ifndef XMEM_HIP_TEMPORAL_H
#define XMEM_HIP_TEMPORAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XMEM_TEMPORAL_MAX_R 7
#define XMEM_TEMPORAL_PRESENT 1    /* flag bit: the frame has a mask; without it the frame neither votes nor changes */
#define XMEM_TEMPORAL_LOCKED 2     /* flag bit: the frame votes for its neighbours but is handed on as it is */
#define XMEM_TEMPORAL_SEGMENT 16   /* output frames one thread walks; a longer call is split in time, each part with its own halo */

/* MAJORITY VOTE over the window t - radius .. t + radius of every pixel of the frames t = t0 .. t0 + n - 1 of a video of T frames
 * of H x W bytes.  Frame t lives in slot t % ring of frames [ring][H][W] (ring == T: the whole video; ring == 2 radius + 1: a delay
 * line fed frame by frame), flags [T] carries the bits above, out [n][H][W] receives the frames and changed [n] the number of
 * pixels of each that differ from the input (overwritten, not added to).
 *   a frame that is not PRESENT, or is LOCKED: out = the input frame, changed = 0;
 *   otherwise, over the PRESENT frames among max(0, t - radius) .. min(T - 1, t + radius): the label that occurs most often at the
 *   pixel; among labels that tie, the frame's own label if it is one of them, else the smallest.
 * Every output frame is computed from input frames only.  `out` MUST NOT overlap `frames`.
 * XMEM_ERR_BAD_ARG: a null pointer, `changed` not 4-byte aligned, radius outside [1, XMEM_TEMPORAL_MAX_R], n < 1, t0 < 0, t0 + n > T, ring < 1, `out` overlapping
 * `frames`, a ring with fewer slots than the frames max(0, t0 - radius) .. min(T - 1, t0 + n - 1 + radius) it must hold at once;
 * XMEM_ERR_UNSUPPORTED: H or W outside [1, 16384], T outside [1, 65535].  Everything is refused before any GPU work. */
int xmem_temporal_mode(const uint8_t* frames, int ring, int H, int W, int T, int t0, int n, int radius, const uint8_t* flags,
                       uint8_t* out, int32_t* changed, void* stream);

#ifdef __cplusplus
}
#endif
#endif
