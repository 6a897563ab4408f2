/*
 * xmem_hip_png.h - seventh header of libxmem_hip.so: finished PNG files of uint8 planes, built on the device, so that only a file's
 * bytes travel to the host.  xmem2_amd/png.py has the definition (`encode_host`) the bytes are held to.
 *
 * The dialect and the conventions are xmem_hip_matte.h's: functions and #defines only, status codes of xmem_hip.h's xmem_status,
 * device pointers, `stream` a hipStream_t passed as void*, scratch passed in and sized by the *_workspace_bytes function, no
 * allocation, no read-back, no host synchronisation, no workgroup waits for another: a call is one memset node and five launches
 * on `stream` and can be captured.  Integer arithmetic; the only atomics are integer OR (token bits into words that rows share)
 * and XOR (CRC-32 partials), whose result depends on no order: the same input gives the same bytes on every run.  xmem_hip.h stays
 * at ABI version 5.
 */
#ifndef XMEM_HIP_PNG_H
#define XMEM_HIP_PNG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XMEM_PNG_META 4            /* int32 words per frame of `meta`: file length, deflate length, 2 spare (zero) */
#define XMEM_PNG_GREY 0            /* colour types, as IHDR names them */
#define XMEM_PNG_RGB 2
#define XMEM_PNG_PALETTE 3
#define XMEM_PNG_MAX_CAPACITY 2147483647   /* of `capacity`, 2^31 - 1: an int's largest; N * capacity may be any size_t */

/* PNG FILES of planes [N][H][W] uint8, one per plane, frame n's at out + n * capacity.
 *   color_type 0: one byte per pixel, table[v] of the plane's byte v (table NULL: v itself);
 *   color_type 3: the same with table [256] required, and palette [256][3] as one PLTE chunk of 256 entries;
 *   color_type 2: three bytes per pixel, table[v][0..2], table [256][3] required.
 * The file is signature, IHDR (8 bit, no interlace), PLTE (type 3), one IDAT, IEND.  IDAT holds a zlib stream 78 01, ONE deflate
 * block with the fixed Huffman codes, the Adler-32.  Every scanline has filter type 2 (Up).  Tokens per row, never across rows: the
 * filter byte a literal; every maximal run of n equal bytes its first byte as a literal, then (n - 1) / 258 matches of length 258
 * at distance 1, then for t = (n - 1) % 258 one match of length t at distance 1 if t >= 3, else t literals.
 * meta[n][0] = the file's true length 63 + D (843 + D with a PLTE), also when it exceeds `capacity`; meta[n][1] = D, the bytes of
 * the deflate block; the other words are 0.  A file longer than 2^31 - 1 bytes reports 2^31 - 1.
 * Bytes of `out` at and beyond `capacity` of a frame keep their values: a frame that did not fit holds its first `capacity`
 * bytes, of which the IDAT checksum is meaningless, and is to be encoded again at its true length.  Shared words are updated with
 * 32-bit atomic ORs of zero bits there, so `out` is 4-byte aligned and its allocation runs to the next multiple of 4 bytes
 * behind out + N * capacity.
 * Steps: a memset of `out`; a row pass (one workgroup per frame and row: the filtered row in LDS, its
 * bit count and Adler partials); a per-frame scan of the bit counts that also writes every byte outside the deflate block but the
 * IDAT checksum; an emit pass (the tokens ORed into an LDS image of the row's bits, then into `out`); a CRC pass (table-driven
 * segments, shifted to their place by multiplication mod the CRC polynomial, XORed together); a last launch for the checksum.
 * XMEM_ERR_BAD_ARG: planes, meta, out or workspace null, meta or out not 4-byte aligned, capacity < 1, a color_type that is not
 * 0, 2 or 3, table null for type 2 or 3, palette null for type 3 or given for another type;
 * XMEM_ERR_UNSUPPORTED: H or W outside [1, 16384], N outside [1, 65535];
 * XMEM_ERR_WORKSPACE: fewer than xmem_png_workspace_bytes(N, H, W, channels) bytes (channels 1 or 3; 0 for arguments outside
 * those ranges), or a workspace that is not 8-byte aligned.  Everything is refused before any GPU work. */
size_t xmem_png_workspace_bytes(int N, int H, int W, int channels);
int xmem_png_encode(const uint8_t* planes, int N, int H, int W, int color_type, const uint8_t* table, const uint8_t* palette,
                    int capacity, int32_t* meta, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
