// pichash.h — the arithmetic of the decoded-picture hashes of --hash 2 (CRC) and --hash 3 (checksum) (x265hip_picture_hash, include/x265hip.h), stated once
// for the kernel (pichash.hip), the binding (x265_amd/host/x265_hip_pichash.cpp) and the CPU checker (tests/support/pichash_ref.cpp).
//
// It restates the reference's updateCRC and updateChecksum (source/common/picyuv.cpp:507-571):
//   CRC        a 16-bit state, polynomial P = x^16 + x^12 + x^5 + 1 (0x1021), no reflection, in AUGMENTED form: every message bit b makes
//              state' = (state * x + b) mod P.  A sample gives its low byte first, bit 7 down to bit 0, then (depth > 8) its high byte: the bytes of the
//              sample as little-endian memory holds them, so a packed plane IS the byte stream.  A byte at a time: s' = T[s >> 8] ^ ((s & 0xff) << 8) ^ b with
//              T[v] = v * x^16 mod P.  A run of N bytes M entered with state s0 leaves s0 * x^(8N) + M(x) mod P: runs combine as
//              v = v_left * x^(8 len_right) + v_right, and leading zero bytes of a run entered with state 0 change nothing.
//   checksum   a sum mod 2^32 over the samples at picture position (x, y): (p & 0xff) ^ mask, and (depth > 8) (p >> 8) ^ mask too, with
//              mask = (uint8_t)((x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8)).  y counts from the top of the PICTURE, not of the band.
// Everything is integer and independent of the order of the parts.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XP_HD __host__ __device__
#else
#define XP_HD
#endif

#define XP_METHOD_CRC       2        /* param->decodedPictureHashSEI */
#define XP_METHOD_CHECKSUM  3
#define XP_POLY             0x1021u

/* the kernel's geometry, in bytes of the packed plane band, counted BACK from the band's end (the short chunk is the first one): a lane folds a chunk, a
 * wave combines 64 of them, a workgroup of four waves a segment.  The tests put their one-hot samples either side of every multiple of these. */
#define XP_CHUNK_BYTES      16
#define XP_WAVE_BYTES       (64 * XP_CHUNK_BYTES)
#define XP_SEGMENT_BYTES    (4 * XP_WAVE_BYTES)

/* one message bit into the state: updateCRC's inner statement */
XP_HD static inline uint32_t xp_crc_bit(uint32_t s, uint32_t bit)
{
    const uint32_t msb = (s >> 15) & 1;
    return (((s << 1) + bit) & 0xffff) ^ (msb * XP_POLY);
}

/* one sample into the state: low byte first, then the high byte when depth > 8 */
XP_HD static inline uint32_t xp_crc_sample(uint32_t s, uint32_t p, int depth)
{
    for (int k = 0; k < 8; k++)
        s = xp_crc_bit(s, (p >> (7 - k)) & 1);
    if (depth > 8)
        for (int k = 0; k < 8; k++)
            s = xp_crc_bit(s, (p >> (15 - k)) & 1);
    return s;
}

/* T[v] = v * x^16 mod P, v < 256 */
XP_HD static inline uint32_t xp_table_entry(uint32_t v)
{
    uint32_t r = v << 8;
    for (int k = 0; k < 8; k++)
        r = ((r << 1) & 0xffff) ^ (((r >> 15) & 1) * XP_POLY);
    return r;
}

/* one message byte into the state, T = the 256 entries above */
template <typename TT>
XP_HD static inline uint32_t xp_crc_byte(uint32_t s, const TT* T, uint32_t b)
{
    return T[s >> 8] ^ ((s & 0xff) << 8) ^ b;
}

/* a * b mod P for polynomials of degree < 16 */
XP_HD static inline uint32_t xp_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int k = 15; k >= 0; k--)
    {
        r = ((r << 1) & 0xffff) ^ (((r >> 15) & 1) * XP_POLY);
        if ((b >> k) & 1)
            r ^= a;
    }
    return r;
}

/* x^k mod P by squaring; k is NOT reduced by any period of x */
XP_HD static inline uint32_t xp_xpow(uint64_t k)
{
    uint32_t r = 1, sq = 2;
    for (; k; k >>= 1)
    {
        if (k & 1)
            r = xp_mul(r, sq);
        sq = xp_mul(sq, sq);
    }
    return r;
}

/* the state after a run of `bytes` message bytes whose value entered with state 0 is `m`, entered with state s0 instead */
XP_HD static inline uint32_t xp_crc_enter(uint32_t s0, uint32_t m, uint64_t bytes)
{
    return xp_mul(s0 & 0xffff, xp_xpow(8 * bytes)) ^ m;
}

XP_HD static inline uint32_t xp_checksum_mask(uint32_t x, uint32_t y)
{
    return ((x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8)) & 0xff;
}

/* the term(s) of the sample p at picture position (x, y) */
XP_HD static inline uint32_t xp_checksum_term(uint32_t p, uint32_t x, uint32_t y, int depth)
{
    const uint32_t mask = xp_checksum_mask(x, y);
    uint32_t t = (p & 0xff) ^ mask;
    if (depth > 8)
        t += (p >> 8) ^ mask;
    return t;
}

/* ---- the host path: plain loops over a strided plane band (plane = the band's first row, stride in samples) */
template <typename P>
static inline uint32_t xp_crc_plane(const P* plane, int64_t stride, int width, int height, int depth, uint32_t state)
{
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            state = xp_crc_sample(state, plane[y * stride + x], depth);
    return state;
}

/* y0 = the picture row of the band's first row */
template <typename P>
static inline uint32_t xp_checksum_plane(const P* plane, int64_t stride, int width, int height, int y0, int depth, uint32_t state)
{
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            state += xp_checksum_term(plane[y * stride + x], (uint32_t)x, (uint32_t)(y0 + y), depth);
    return state;
}

template <typename P>
static inline uint32_t xp_hash_plane(int method, const P* plane, int64_t stride, int width, int height, int y0, int depth, uint32_t state)
{
    return method == XP_METHOD_CRC ? xp_crc_plane(plane, stride, width, height, depth, state) : xp_checksum_plane(plane, stride, width, height, y0, depth, state);
}
