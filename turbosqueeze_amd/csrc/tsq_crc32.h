// tsq_crc32.h -- zlib's CRC-32 (polynomial 0xEDB88320, reflected), for host and device code alike: the arithmetic mod P and the
// tables that follow from it, no kernels.  Written here; nothing of libz is linked or copied.
//
// The convention is zlib's: bit 31 of a word is x^0, so the polynomial 1 is 0x80000000 and x^8 is 0x00800000.  R(M) is the CRC
// register behind the bytes M with init 0 and no final xor; it is M(x) * x^32 mod P, hence linear:
//   R(0...0 | M) = R(M)                                    zeros in front do not count
//   R(A | B)     = R(A) (x) x^(8 |B|)  xor  R(B)
//   crc32(M)     = R(M)  xor  0xFFFFFFFF (x) x^(8 |M|)  xor  0xFFFFFFFF
//   crc32(A | B) = crc32(A) (x) x^(8 |B|)  xor  crc32(B)   (tsqa_crc32_combine)
// x has order 2^32 - 1 mod P, so exponents may be reduced mod 2^32 - 1, and x^(-k) is x^(2^32 - 1 - k).
#pragma once

#include "tsq_common.cuh"

namespace tsq {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcOne = 0x80000000u;                    // the polynomial 1
constexpr uint32_t kCrcX8 = 0x00800000u;                     // x^8

// a (x) b: the product mod P, 32 steps without a branch (step i: b where bit 31 - i of a is set -- the sign of a << i spread over
// the word --, then b times x).  The ONE product: the decoder's flush, the fold kernel, the host's combine and the tables use it.
__host__ __device__ __forceinline__ constexpr uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
#pragma unroll
    for (uint32_t i = 0; i < 32u; ++i) {
        r ^= b & (uint32_t)((int32_t)(a << i) >> 31);
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
    }
    return r;
}

// x^(8 n) for a byte count n of 64 bits: 8 n passes 2^32 at 512 MiB, so the count is reduced mod 2^32 - 1 first (2^32 = 1 there,
// so the halves of n simply add), and the 35-bit exponent 8 n is walked by square and multiply from x^8
__host__ __device__ constexpr uint32_t crc_xpow8(uint64_t n)
{
    n = (n >> 32) + (n & 0xFFFFFFFFull);                     // < 2^33, the same mod 2^32 - 1
    n = (n >> 32) + (n & 0xFFFFFFFFull);                     // <= 2^32
    uint32_t r = kCrcOne, b = kCrcX8;
    while (n) {
        if (n & 1u) r = crc_mul(r, b);
        b = crc_mul(b, b);
        n >>= 1;
    }
    return r;
}

// x^(-8 n), 0 <= n < 2^29: the inverse of x^(8 n)
__host__ __device__ constexpr uint32_t crc_xpow8_inverse(uint32_t n) { return crc_xpow8(0xFFFFFFFFull - n); }

// What crc32 adds to R for a message of n bytes: the init word carried to the end, and the final xor
__host__ __device__ constexpr uint32_t crc_init_term(uint64_t n) { return crc_mul(0xFFFFFFFFu, crc_xpow8(n)) ^ 0xFFFFFFFFu; }

// R(byte | k zero bytes) for k = 0: eight steps of the register
__host__ __device__ constexpr uint32_t crc_byte(uint32_t byte)
{
    uint32_t c = byte;
    for (uint32_t k = 0; k < 8u; ++k) c = (c >> 1) ^ ((c & 1u) ? kCrcPoly : 0u);
    return c;
}

// The tables the decoder's CRC flush keeps in LDS (tsq_dec_common.cuh, flush_crc), made once at compile time:
//   slice[k][b], k < 4: R(b | k zero bytes) -- four look-ups take a register over four bytes
//   pow[k], k <= kCrcCells: x^(128 k), the shift over k cells of 16 bytes
//   inv[r], r < 16: x^(-8 r), which takes the zero bytes behind a block's last byte off again
constexpr uint32_t kCrcCells = 770u;                         // an image of OUTC bytes touches at most 769 cells
struct CrcTables {
    uint32_t slice[4][256];
    uint32_t pow[kCrcCells + 1u];
    uint32_t inv[16];
};
constexpr uint32_t kCrcLdsWords = 4u * 256u + kCrcCells + 1u;   // slice and pow go to LDS, in this order

constexpr CrcTables crc_make_tables()
{
    CrcTables t = {};
    for (uint32_t b = 0; b < 256u; ++b) t.slice[0][b] = crc_byte(b);
    for (uint32_t k = 1; k < 4u; ++k)
        for (uint32_t b = 0; b < 256u; ++b) { const uint32_t c = t.slice[k - 1u][b]; t.slice[k][b] = (c >> 8) ^ t.slice[0][c & 0xFFu]; }
    const uint32_t x128 = crc_xpow8(16);
    t.pow[0] = kCrcOne;
    for (uint32_t k = 1; k <= kCrcCells; ++k) t.pow[k] = crc_mul(t.pow[k - 1u], x128);
    const uint32_t x8_inverse = crc_xpow8_inverse(1);
    t.inv[0] = kCrcOne;
    for (uint32_t r = 1; r < 16u; ++r) t.inv[r] = crc_mul(t.inv[r - 1u], x8_inverse);
    return t;
}

// the device's copy (a unit that launches no CRC kernel drops it)
static __device__ const CrcTables g_crc_tables = crc_make_tables();

// zlib's crc32(crc, buf, n) on the host, a byte at a time through slice[0] (callers: tsqa_crc32_host, tsqa_plan_crc32)
inline uint32_t crc_update_host(const CrcTables& t, uint32_t crc, const uint8_t* p, size_t n)
{
    uint32_t c = ~crc;
    while (n >= 4u) {
        c ^= (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        c = t.slice[3][c & 0xFFu] ^ t.slice[2][(c >> 8) & 0xFFu] ^ t.slice[1][(c >> 16) & 0xFFu] ^ t.slice[0][c >> 24];
        p += 4; n -= 4u;
    }
    while (n--) c = (c >> 8) ^ t.slice[0][(c ^ *p++) & 0xFFu];
    return ~c;
}

}  // namespace tsq
