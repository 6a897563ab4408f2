/*
 * xmem_hip_polygons.h - third header of libxmem_hip.so: the polygon outlines (rings of corners) of uint8 index masks, traced on the
 * device.
 *
 * The dialect and the conventions are xmem_hip_masks.h's: functions and #defines only, status codes of xmem_hip.h's xmem_status,
 * device pointers, `stream` a hipStream_t passed as void*, scratch passed in and sized by the *_workspace_bytes function, no
 * allocation, no read-back, no host synchronisation: a call is a sequence of launches on `stream` whose number depends on
 * (N, H, W, K, capacity) alone, and can be captured.  Integer arithmetic; the only atomics are integer sums: the same input gives
 * the same bytes on every run.  xmem_hip.h stays at ABI version 5.
 */
#ifndef XMEM_HIP_POLYGONS_H
#define XMEM_HIP_POLYGONS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* meta [N][K][XMEM_POLY_META] int32 */
#define XMEM_POLY_META 2
#define XMEM_POLY_CORNERS 0
#define XMEM_POLY_RINGS 1
/* a corner word: x | y << 16 | first corner of its ring << 31 */
#define XMEM_POLY_FIRST_BIT 31
#define XMEM_POLY_MAX_CAPACITY 268435456

/* POLYGON OUTLINES of the labels 1..K of index maps masks [N][H][W] (labels above K are ignored), xmem2_amd/polygons.py has the
 * definition: lattice vertices (x, y), 0 <= x <= W, 0 <= y <= H; the boundary of {m == k} as directed unit edges with the region
 * on the right (x to the right, y down); at a vertex where two diagonal pixels meet the two pixels are joined (the region is
 * 8-connected); a ring is the list of its corners in travelling order from its corner with the smallest (y, x), the rings of a
 * label are ordered by that corner.
 *   meta [n][k - 1] = {corners, rings} of label k: the TRUE counts, whether or not the corners fitted;
 *   corners [n][capacity] uint32: the corner lists of the labels 1, 2, .., K back to back, one word per corner.  Nothing is written
 *   at or beyond `capacity`; for a frame whose corners did not fit (sum of the counts > capacity) only `meta` is meaningful.
 * Steps: the 8-connected components of the map (xmem_components: the number of outer rings of a label is its number of
 * components, the number of its holes follows from the turns counted at the corners); a walk along the lattice rows that counts
 * corners per (label, row) and (label, column); a scan; a walk along the rows and one along the columns that give every corner its
 * rank in row-major and column-major order - a ring alternates horizontal and vertical edges, the corners of a label on one lattice
 * line pair up in sorted order, so the predecessor of a corner is its neighbour in one of the two orders; pointer jumping over the
 * corners (the ring's smallest corner and the distance to it), a scan over the ring lengths and the emit - one launch with a
 * workgroup per frame in LDS when capacity <= 4096, else ceil(log2(min(capacity, 4 (H + 1) (W + 1)))) rounds on global arrays.
 * N in [1, 65535], K in [1, 254], capacity in [1, XMEM_POLY_MAX_CAPACITY], no null pointer (else XMEM_ERR_BAD_ARG); H, W in
 * [1, 16384] (else XMEM_ERR_UNSUPPORTED); workspace: xmem_mask_polygons_workspace_bytes(N, H, W, K, capacity) bytes (0 for arguments
 * outside those ranges), 8-byte aligned (a smaller one: XMEM_ERR_WORKSPACE).  Everything is refused before any GPU work. */
size_t xmem_mask_polygons_workspace_bytes(int N, int H, int W, int K, int capacity);
int xmem_mask_polygons(const uint8_t* masks, int N, int H, int W, int K, int capacity, int32_t* meta, uint32_t* corners,
                       void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
