/*
 * xmem_hip_matte.h - fifth header of libxmem_hip.so: a capped, signed, per-label squared distance on uint8 index masks, and what is
 * looked up in it or searched with it: feathered mattes and trimaps, grow and shrink.  xmem2_amd/matte.py has the definitions.
 *
 * The dialect and the conventions are xmem_hip_masks.h's: functions and #defines only, status codes of xmem_hip.h's xmem_status,
 * device pointers, `stream` a hipStream_t passed as void*, scratch passed in and sized by the *_workspace_bytes function, no
 * allocation, no read-back, no host synchronisation: a call is two launches on `stream` and can be captured.  Integer arithmetic,
 * no atomics: the same input gives the same bytes on every run.  xmem_hip.h stays at ABI version 5.
 *
 * Distances run between pixel centres and NOTHING exists outside the image: an object that touches the border has no edge there
 * (xmem_edt_sq puts a ring of zeros round the image; this header does not).  Both passes are capped: the column pass looks no
 * further than R + 1 rows, the row pass no further than R columns.
 */
#ifndef XMEM_HIP_MATTE_H
#define XMEM_HIP_MATTE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XMEM_MATTE_MAX_R 127
#define XMEM_MATTE_MAX_TABLES 4
#define XMEM_MATTE_MAX_LABELS 255

/* SIGNED SQUARED DISTANCE of the labels k = 1..K of index maps masks [N][H][W] into out [N][K][H][W] int32, cap2 = (R + 1)^2:
 *   out[n][k-1](p) = +min(cap2, min over q of frame n with m(q) != k of |p - q|^2)   where m(p) == k,
 *                    -min(cap2, min over q of frame n with m(q) == k of |p - q|^2)   elsewhere;    a minimum over no pixel is cap2.
 * Steps: a column pass writes one byte per (frame, label, pixel) into the workspace - the distance, capped at R + 1, to the
 * nearest pixel of its column on the other side of `m == k`; a row pass keeps the squares of one row in LDS and every pixel
 * searches outwards from its column while dx^2 is below the best it has.
 * N in [1, 65535], K in [1, XMEM_MATTE_MAX_LABELS], R in [1, XMEM_MATTE_MAX_R], no null pointer, out 4-byte aligned (else
 * XMEM_ERR_BAD_ARG); H, W in [1, 16384] (else XMEM_ERR_UNSUPPORTED); workspace: xmem_signed_edt_workspace_bytes(N, H, W, K) bytes
 * (0 for arguments outside those ranges), 8-byte aligned (a smaller one: XMEM_ERR_WORKSPACE).  Everything is refused before any
 * GPU work. */
size_t xmem_signed_edt_workspace_bytes(int N, int H, int W, int K);
int xmem_signed_edt(const uint8_t* masks, int N, int H, int W, int K, int R, int32_t* out, void* workspace, size_t workspace_bytes,
                    void* stream);

/* LOOK-UPS in that distance: out [T][N][K][H][W] uint8 = tables[t][s2 + cap2] with tables [T][2 * cap2 + 1] uint8 and s2 what
 * xmem_signed_edt gives.  One distance computation serves the T tables (a matte and a trimap come from one pass); the look-up is
 * part of the row pass and no int32 plane is written.  T in [1, XMEM_MATTE_MAX_TABLES] (else XMEM_ERR_BAD_ARG), the rest as
 * xmem_signed_edt; workspace: xmem_mask_matte_workspace_bytes(N, H, W, K). */
size_t xmem_mask_matte_workspace_bytes(int N, int H, int W, int K);
int xmem_mask_matte(const uint8_t* masks, int N, int H, int W, int K, int R, const uint8_t* tables, int T, uint8_t* out,
                    void* workspace, size_t workspace_bytes, void* stream);

/* GROW (shrink == 0) or SHRINK (shrink != 0) of index maps masks [N][H][W] into out [N][H][W] by the squared radius r2.
 *   grow:   out(p) = m(p) where m(p) != 0 (objects never eat one another); else the label of the object pixel q with
 *           |p - q|^2 <= r2 that minimises (|p - q|^2, m(q)) lexicographically - ties go to the smaller label -, 0 without one.
 *   shrink: out(p) = 0 where m(p) != 0 and some q with m(q) != m(p) has |p - q|^2 <= r2; else m(p).
 * Grow carries (distance, label) through both passes; shrink uses the distance to the end of a pixel's vertical run of equal
 * values, which depends on no label.  `out` MUST NOT overlap `masks` (XMEM_ERR_BAD_ARG).  r2 in [1, XMEM_MATTE_MAX_R^2], N, H, W,
 * the codes and the alignment as above; workspace: xmem_mask_grow_workspace_bytes(N, H, W). */
size_t xmem_mask_grow_workspace_bytes(int N, int H, int W);
int xmem_mask_grow(const uint8_t* masks, int N, int H, int W, int r2, int shrink, uint8_t* out, void* workspace,
                   size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
