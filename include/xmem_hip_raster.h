/*
 * xmem_hip_raster.h - fourth header of libxmem_hip.so: polygons filled back into uint8 index masks on the device, the reader of
 * what xmem_hip_polygons.h writes and of polygon annotations (labelme, COCO `segmentation` lists).
 *
 * The dialect and the conventions are xmem_hip_masks.h's: functions and #defines only, status codes of xmem_hip.h's xmem_status,
 * device pointers, `stream` a hipStream_t passed as void*, scratch passed in and sized by the *_workspace_bytes function, no
 * allocation, no read-back, no host synchronisation: a call is a sequence of launches on `stream` whose number depends on
 * (E, N, H, W, R) alone, and can be captured.  Integer arithmetic; the only atomics are XORs of single bits, which commute: the
 * same input gives the same bytes on every run.  xmem_hip.h stays at ABI version 5.
 */
#ifndef XMEM_HIP_RASTER_H
#define XMEM_HIP_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XMEM_FILL_MAX_FRAC_BITS 8
/* a coordinate's magnitude, in units of 1 / 2^frac_bits pixel: every product of the rule stays below 2^62 */
#define XMEM_FILL_COORD_BOUND 268435456
/* status [2] int32: edges skipped for their plane index, edges skipped for a coordinate */
#define XMEM_FILL_STATUS 2
#define XMEM_FILL_BAD_PLANE 0
#define XMEM_FILL_BAD_COORD 1

/* EVEN-ODD FILL of polygon edges into index maps masks [N][H][W], xmem2_amd/polygons.py (`fill_exact_host`, `fill_rows_host`) has
 * the definition.  edges [E][4] int32 = xa, ya, xb, yb in units of 1 / one pixel, one = 2^frac_bits, with ya < yb (an edge with
 * ya >= yb takes no part); plane [E] = frame * R + row.  Pixel (r, c) is the unit square whose centre is (c + 1/2, r + 1/2).  An
 * edge crosses image row r when 2 ya <= (2 r + 1) one < 2 yb and toggles the first column whose centre is at or right of it:
 * c = ceil(num / den), num = 2 xa dy + ((2 r + 1) one - 2 ya) dx - one dy, den = 2 one dy, clipped to [0, W]; a pixel is inside a
 * row's polygons when the running parity of the toggles along its image row is odd.  The pixel gets values[row] (values NULL:
 * row + 1) of the HIGHEST row that contains it; a pixel in no row is set to 0, or with overlay != 0 left as it is.
 * An edge whose plane index is outside [0, N R) or one of whose coordinates exceeds XMEM_FILL_COORD_BOUND in magnitude is skipped,
 * counted in status [XMEM_FILL_STATUS] and dereferences nothing.
 * Steps: the workspace - one bit per (frame, row, image row, column 0..W), N R H ceil((W + 1) / 32) words - and status are cleared;
 * a grid sized by E alone in which a lane owns an edge, walks its clipped rows (quotient and remainder of num / den are stepped,
 * one division per walk) and XORs one bit per crossing, the long edges of a wave being walked by all 64 lanes; a grid over the
 * image rows that runs the prefix XOR along each line, picks the highest row and writes the bytes.  With E == 0 the planes are
 * still cleared, or kept under overlay.
 * E >= 0, N in [1, 65535], R in [1, 254], frac_bits in [0, XMEM_FILL_MAX_FRAC_BITS], no null pointer but `values` (and edges, plane
 * when E == 0), status 4-byte aligned (else XMEM_ERR_BAD_ARG); H, W in [1, 16384] (else XMEM_ERR_UNSUPPORTED); workspace:
 * xmem_polygons_fill_workspace_bytes(N, H, W, R) bytes (0 for arguments outside those ranges), 8-byte aligned (a smaller one:
 * XMEM_ERR_WORKSPACE).  Everything is refused before any GPU work. */
size_t xmem_polygons_fill_workspace_bytes(int N, int H, int W, int R);
int xmem_polygons_fill(const int32_t* edges, const int32_t* plane, int E, int N, int H, int W, int R, int frac_bits,
                       const uint8_t* values, int overlay, uint8_t* masks, int32_t* status, void* workspace, size_t workspace_bytes,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
