/*
 * xmem_hip_motion.h - ninth header of libxmem_hip.so: 8-bit luma, an exhaustive integer block-motion search and the
 * motion-compensated majority vote along the time axis of uint8 index masks.  xmem2_amd/motion.py (`luma_host`,
 * `block_motion_host`) and xmem2_amd/temporal.py (`mode_mc_host`) have the definitions the bytes are held to.
 *
 * The dialect and the conventions are xmem_hip_temporal.h's: functions and #defines only, status codes of xmem_hip.h's xmem_status,
 * device pointers, `stream` a hipStream_t passed as void*, no allocation, no read-back, no host synchronisation: every call can be
 * captured.  Integer arithmetic; a search result is a minimum, which depends on no order, and the only atomics are the integer adds
 * into `changed`: the same input gives the same bytes on every run.  xmem_hip.h stays at ABI version 5.
 *
 * NOTHING exists outside an image or the video: a displaced block lies wholly inside the reference frame or is no candidate, a
 * window is clipped at frame 0 and at frame T - 1.  Blocks are XMEM_MOTION_BLOCK pixels square; those of the last row and column
 * are cropped to the image.  By = ceil(H / XMEM_MOTION_BLOCK), Bx = ceil(W / XMEM_MOTION_BLOCK).
 */
#ifndef XMEM_HIP_MOTION_H
#define XMEM_HIP_MOTION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XMEM_MOTION_BLOCK 16
#define XMEM_MOTION_MAX_SEARCH 32
#define XMEM_MOTION_MAX_N 65535    /* images, or pairs, of one call */

/* LUMA of N frames of H x W RGB bytes: rgb [N][H][W][3] -> out [N][H][W], (77 R + 150 G + 29 B + 128) >> 8.
 * XMEM_ERR_BAD_ARG: a null pointer, N < 1; XMEM_ERR_UNSUPPORTED: H or W outside [1, 16384], N above XMEM_MOTION_MAX_N. */
int xmem_luma_u8(const uint8_t* rgb, int N, int H, int W, uint8_t* out, void* stream);

/* BLOCK MOTION of N independent pairs: cur, ref [N][H][W] -> vec [N][By][Bx][2] as (dy, dx), sad [N][By][Bx].  The candidates of a
 * block are the (dy, dx) in [-search, search]^2 whose displaced (cropped) block lies inside ref; the winner minimises (SAD,
 * dy^2 + dx^2, dy, dx) in that order; if SAD(0, 0) - SAD(winner) <= bias * pixels of the block, the block takes (0, 0) and SAD(0, 0).
 * One launch.  XMEM_ERR_BAD_ARG: a null pointer, `sad` not 4-byte aligned, N < 1, search outside [1, XMEM_MOTION_MAX_SEARCH], bias
 * outside [0, 255]; XMEM_ERR_UNSUPPORTED: H or W outside [1, 16384], N above XMEM_MOTION_MAX_N. */
int xmem_block_motion(const uint8_t* cur, const uint8_t* ref, int N, int H, int W, int search, int bias, int8_t* vec, int32_t* sad,
                      void* stream);

/* BLOCK MOTION of a window of a video of T frames of lumas: frame t lives in slot t % ring of luma [ring][H][W], flags [T] carries
 * the bits of xmem_hip_temporal.h (1 present, 2 locked).  For every output frame t = t0 .. t0 + n - 1 and every offset j = -radius ..
 * -1, +1 .. +radius (entry e = j + radius for j < 0, j + radius - 1 for j > 0) the search of frame t (cur) in frame t + j (ref):
 * vec [n][2 radius][By][Bx][2], sad [n][2 radius][By][Bx].  sad = -1 and vec = 0 where t + j is outside the video, where t + j is not
 * present, and where t itself is not present or is locked.  One launch, the search of xmem_block_motion.
 * XMEM_ERR_BAD_ARG: as xmem_block_motion, and radius outside [1, 7], n < 1, t0 < 0, t0 + n > T, ring < 1, a ring with fewer slots
 * than the frames max(0, t0 - radius) .. min(T - 1, t0 + n - 1 + radius); XMEM_ERR_UNSUPPORTED: H or W outside [1, 16384], T outside
 * [1, 65535]. */
int xmem_motion_window(const uint8_t* luma, int ring, int H, int W, int T, int t0, int n, int radius, const uint8_t* flags, int search,
                       int bias, int8_t* vec, int32_t* sad, void* stream);

/* MOTION-COMPENSATED MAJORITY VOTE: xmem_temporal_mode with every neighbour aligned block by block.  frames, ring, T, t0, n, radius,
 * flags, out [n][H][W] and changed [n] are xmem_temporal_mode's; vec and sad are what xmem_motion_window wrote for the same t0, n
 * and radius.  The vote of frame t + j at pixel p is frames[t + j][p + vec of p's block]; an entry with sad < 0 or sad > max_sad *
 * pixels of the block does not vote at that block's pixels; the centre always votes.  The key is xmem_temporal_mode's.  A vector
 * that would leave the frame (never one of xmem_motion_window's) makes its entry abstain.  One memset node and one launch.
 * XMEM_ERR_BAD_ARG: a null pointer, `changed` or `sad` not 4-byte aligned, radius outside [1, 7], max_sad outside [0, 255], n < 1,
 * t0 < 0, t0 + n > T, ring < 1, `out` overlapping `frames`, a ring too small (as above); XMEM_ERR_UNSUPPORTED: H or W outside
 * [1, 16384], T outside [1, 65535]. */
int xmem_temporal_mode_mc(const uint8_t* frames, int ring, int H, int W, int T, int t0, int n, int radius, const uint8_t* flags,
                          const int8_t* vec, const int32_t* sad, int max_sad, uint8_t* out, int32_t* changed, void* stream);

#ifdef __cplusplus
}
#endif
#endif
