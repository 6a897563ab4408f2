/*
 * xmem_hip_masks.h - second header of libxmem_hip.so: connected components and the clean-up of uint8 index masks on the device.
 *
 * xmem_hip.h is frozen at ABI version 5 (its symbols, structs and that number); entry points added after it are declared here, in
 * the same dialect (xmem2_amd/_header.py reads both), with functions and #defines only: no struct crosses this part of the ABI.
 * Status codes are xmem_hip.h's xmem_status (0 on success, negative otherwise), the conventions are the ones stated there: device
 * pointers, `stream` a hipStream_t passed as void*, scratch passed in and sized by the matching *_workspace_bytes function, no
 * allocation, no read-back, no host synchronisation: every call is a fixed sequence of launches on `stream` and can be captured.
 * Everything is integer arithmetic with integer atomics whose result does not depend on their order: the same input gives the same
 * bytes on every run.
 */
#ifndef XMEM_HIP_MASKS_H
#define XMEM_HIP_MASKS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* index of xmem_mask_clean's per-frame counters: stats [N][XMEM_CLEAN_STATS] */
#define XMEM_CLEAN_STATS 4
#define XMEM_CLEAN_COMPONENTS_REMOVED 0
#define XMEM_CLEAN_PIXELS_REMOVED 1
#define XMEM_CLEAN_HOLES_FILLED 2
#define XMEM_CLEAN_PIXELS_FILLED 3

/* CONNECTED COMPONENTS of uint8 maps masks [N][H][W].  A component is a maximal set of pixels of EQUAL value (0 is a value like any
 * other) that is 4- or 8-connected (`connectivity`).  root [N][H][W]: the row-major index y * W + x, within the frame, of the first
 * pixel of the pixel's component; area [N][H][W]: the component's number of pixels.  Union-find: a workgroup resolves a 32 x 32
 * tile in LDS, a second kernel unites across the tile borders with atomicMin on the parent array (the larger root is always linked
 * under the smaller, so the surviving root is the component's smallest index whatever order the atomics arrive in), a third flattens
 * and adds up the areas (counted per tile in LDS, one global add per tile and component), a fourth hands every pixel its area.
 * N in [1, 65535], connectivity 4 or 8, no null pointer (else XMEM_ERR_BAD_ARG); H, W in [1, 16384] (else XMEM_ERR_UNSUPPORTED);
 * workspace: xmem_components_workspace_bytes(N, H, W) bytes (0 for arguments outside those ranges), 8-byte aligned (a smaller one:
 * XMEM_ERR_WORKSPACE).  Everything is refused before any GPU work. */
size_t xmem_components_workspace_bytes(int N, int H, int W);
int xmem_components(const uint8_t* masks, int N, int H, int W, int connectivity, int32_t* root, int32_t* area, void* workspace,
                    size_t workspace_bytes, void* stream);

/* MASK CLEAN-UP of index maps masks [N][H][W] (0 background, labels 1..255) into out [N][H][W], two passes.
 *   A, objects: the 8-connected components of the labels >= 1.  A component is set to 0 if keep_largest != 0 and it is not the
 *      largest of its label in its frame (of equal areas the one with the smaller root is the largest), or if its area < min_area.
 *   B, holes, only with max_hole > 0, on the result of A: a 4-connected component of value 0 is filled with the label k if it
 *      touches no border pixel of the image, its area <= max_hole, and every 4-neighbour of its pixels outside it carries k.
 * stats [N][XMEM_CLEAN_STATS] int32: components removed, pixels removed, holes filled, pixels filled, per frame (overwritten).
 * `out` MUST NOT overlap `masks` (XMEM_ERR_BAD_ARG): pass B reads neighbours of what pass A wrote.
 * min_area, max_hole >= 0, and the ranges, codes and alignment of xmem_components; workspace: xmem_mask_clean_workspace_bytes. */
size_t xmem_mask_clean_workspace_bytes(int N, int H, int W);
int xmem_mask_clean(const uint8_t* masks, int N, int H, int W, int min_area, int max_hole, int keep_largest, uint8_t* out,
                    int32_t* stats, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
