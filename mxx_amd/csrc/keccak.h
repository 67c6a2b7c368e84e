/* keccak.h — a Keccak-f[1600] sponge of rate 136 (Keccak-256 and SHA3-256), for host and device code alike.
 *
 * hash_seed_for_matrix of the reference (src/sampler/gpu.rs:118-136) turns a key and a tag into a sampler seed with one
 * 32-byte digest; hash_seed.hip runs it with one lane per tag.  What that needs of a sponge, and what shapes this text:
 *   - the state is 25 uint64_t addressed by constants only, the 24 rounds written out, the round constants immediates:
 *     nothing is indexed by a run-time value, so on the device the state lives in registers and nowhere else;
 *   - the message is never laid out in memory.  The absorber asks a functor `byte_at(pos)` for byte `pos` of the message
 *     and assembles the 17 lanes of a rate block one by one, each with its lane index known at compile time;
 *   - the padding byte is an argument: 0x01 is Keccak-256 (the original padding, what keccak_asm::Keccak256 computes),
 *     0x06 is SHA3-256.  The closing bit 0x80 is OR-ed into the last byte of the last block, which is also the padding
 *     byte's place when the message is one byte short of a block boundary;
 *   - a message of any length: len / 136 + 1 blocks;
 *   - the first four lanes are squeezed, the 32-byte digest read as little-endian words.
 *
 * Plain C++17: a host program that includes this file alone compiles it without HIP (tests/cpp/keccak_check.cpp).
 */
#ifndef MXX_KECCAK_H
#define MXX_KECCAK_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KECCAK_FN __host__ __device__ static inline
#else
#define KECCAK_FN static inline
#endif

#define KECCAK_RATE 136 /* bytes: 17 lanes; capacity 512 bits */
#define KECCAK_PAD_KECCAK256 0x01
#define KECCAK_PAD_SHA3_256 0x06

#define KECCAK_ROL(v, n) (((v) << (n)) | ((v) >> (64 - (n))))

/* one round on a[0..24] (lane (x, y) at a[x + 5 y]): theta, rho and pi into b, chi back into a, iota */
#define KECCAK_CHI_ROW(o)                     \
    a[o + 0] = b##o##0 ^ (~b##o##1 & b##o##2); \
    a[o + 1] = b##o##1 ^ (~b##o##2 & b##o##3); \
    a[o + 2] = b##o##2 ^ (~b##o##3 & b##o##4); \
    a[o + 3] = b##o##3 ^ (~b##o##4 & b##o##0); \
    a[o + 4] = b##o##4 ^ (~b##o##0 & b##o##1);

#define KECCAK_ROUND(RC)                                                                  \
    do {                                                                                  \
        const uint64_t c0 = a[0] ^ a[5] ^ a[10] ^ a[15] ^ a[20];                          \
        const uint64_t c1 = a[1] ^ a[6] ^ a[11] ^ a[16] ^ a[21];                          \
        const uint64_t c2 = a[2] ^ a[7] ^ a[12] ^ a[17] ^ a[22];                          \
        const uint64_t c3 = a[3] ^ a[8] ^ a[13] ^ a[18] ^ a[23];                          \
        const uint64_t c4 = a[4] ^ a[9] ^ a[14] ^ a[19] ^ a[24];                          \
        const uint64_t d0 = c4 ^ KECCAK_ROL(c1, 1), d1 = c0 ^ KECCAK_ROL(c2, 1);          \
        const uint64_t d2 = c1 ^ KECCAK_ROL(c3, 1), d3 = c2 ^ KECCAK_ROL(c4, 1);          \
        const uint64_t d4 = c3 ^ KECCAK_ROL(c0, 1);                                       \
        /* b<5y><x> = lane (x, y) after rho and pi: B[y][2x + 3y] = rol(A[x][y], r[x][y]) */ \
        const uint64_t t0 = a[0] ^ d0, b00 = t0;                                          \
        const uint64_t t1 = a[6] ^ d1, b01 = KECCAK_ROL(t1, 44);                          \
        const uint64_t t2 = a[12] ^ d2, b02 = KECCAK_ROL(t2, 43);                         \
        const uint64_t t3 = a[18] ^ d3, b03 = KECCAK_ROL(t3, 21);                         \
        const uint64_t t4 = a[24] ^ d4, b04 = KECCAK_ROL(t4, 14);                         \
        const uint64_t t5 = a[3] ^ d3, b50 = KECCAK_ROL(t5, 28);                          \
        const uint64_t t6 = a[9] ^ d4, b51 = KECCAK_ROL(t6, 20);                          \
        const uint64_t t7 = a[10] ^ d0, b52 = KECCAK_ROL(t7, 3);                          \
        const uint64_t t8 = a[16] ^ d1, b53 = KECCAK_ROL(t8, 45);                         \
        const uint64_t t9 = a[22] ^ d2, b54 = KECCAK_ROL(t9, 61);                         \
        const uint64_t t10 = a[1] ^ d1, b100 = KECCAK_ROL(t10, 1);                        \
        const uint64_t t11 = a[7] ^ d2, b101 = KECCAK_ROL(t11, 6);                        \
        const uint64_t t12 = a[13] ^ d3, b102 = KECCAK_ROL(t12, 25);                      \
        const uint64_t t13 = a[19] ^ d4, b103 = KECCAK_ROL(t13, 8);                       \
        const uint64_t t14 = a[20] ^ d0, b104 = KECCAK_ROL(t14, 18);                      \
        const uint64_t t15 = a[4] ^ d4, b150 = KECCAK_ROL(t15, 27);                       \
        const uint64_t t16 = a[5] ^ d0, b151 = KECCAK_ROL(t16, 36);                       \
        const uint64_t t17 = a[11] ^ d1, b152 = KECCAK_ROL(t17, 10);                      \
        const uint64_t t18 = a[17] ^ d2, b153 = KECCAK_ROL(t18, 15);                      \
        const uint64_t t19 = a[23] ^ d3, b154 = KECCAK_ROL(t19, 56);                      \
        const uint64_t t20 = a[2] ^ d2, b200 = KECCAK_ROL(t20, 62);                       \
        const uint64_t t21 = a[8] ^ d3, b201 = KECCAK_ROL(t21, 55);                       \
        const uint64_t t22 = a[14] ^ d4, b202 = KECCAK_ROL(t22, 39);                      \
        const uint64_t t23 = a[15] ^ d0, b203 = KECCAK_ROL(t23, 41);                      \
        const uint64_t t24 = a[21] ^ d1, b204 = KECCAK_ROL(t24, 2);                       \
        KECCAK_CHI_ROW(0)                                                                 \
        KECCAK_CHI_ROW(5)                                                                 \
        KECCAK_CHI_ROW(10)                                                                \
        KECCAK_CHI_ROW(15)                                                                \
        KECCAK_CHI_ROW(20)                                                                \
        a[0] ^= UINT64_C(RC);                                                             \
    } while (0)

KECCAK_FN void keccak_f1600(uint64_t a[25]) {
    KECCAK_ROUND(0x0000000000000001);
    KECCAK_ROUND(0x0000000000008082);
    KECCAK_ROUND(0x800000000000808A);
    KECCAK_ROUND(0x8000000080008000);
    KECCAK_ROUND(0x000000000000808B);
    KECCAK_ROUND(0x0000000080000001);
    KECCAK_ROUND(0x8000000080008081);
    KECCAK_ROUND(0x8000000000008009);
    KECCAK_ROUND(0x000000000000008A);
    KECCAK_ROUND(0x0000000000000088);
    KECCAK_ROUND(0x0000000080008009);
    KECCAK_ROUND(0x000000008000000A);
    KECCAK_ROUND(0x000000008000808B);
    KECCAK_ROUND(0x800000000000008B);
    KECCAK_ROUND(0x8000000000008089);
    KECCAK_ROUND(0x8000000000008003);
    KECCAK_ROUND(0x8000000000008002);
    KECCAK_ROUND(0x8000000000000080);
    KECCAK_ROUND(0x000000000000800A);
    KECCAK_ROUND(0x800000008000000A);
    KECCAK_ROUND(0x8000000080008081);
    KECCAK_ROUND(0x8000000000008080);
    KECCAK_ROUND(0x0000000080000001);
    KECCAK_ROUND(0x8000000080008008);
}

/* byte `pos` of the padded message: the message, then the padding byte, zeros, and 0x80 OR-ed into the last byte
 * (pos == last) of the last block */
template <typename ByteAt>
KECCAK_FN uint64_t keccak_padded_byte(const ByteAt &byte_at, size_t len, uint8_t pad, size_t last, size_t pos) {
    uint64_t v = pos < len ? byte_at(pos) : (pos == len ? pad : 0);
    if (pos == last) v |= 0x80;
    return v;
}

/* the 8 bytes from `pos` on as a little-endian lane */
template <typename ByteAt>
KECCAK_FN uint64_t keccak_lane(const ByteAt &byte_at, size_t len, uint8_t pad, size_t last, size_t pos) {
    uint64_t v = 0;
    if (pos + 8 <= len) { /* inside the message: no padding to look for */
        for (int k = 0; k < 8; ++k) v |= static_cast<uint64_t>(byte_at(pos + k)) << (8 * k);
    } else {
        for (int k = 0; k < 8; ++k) v |= keccak_padded_byte(byte_at, len, pad, last, pos + k) << (8 * k);
    }
    return v;
}

/* digest[0..3] = the first four state lanes after absorbing the `len` bytes byte_at(0) .. byte_at(len - 1) under the
 * padding byte `pad`: bytes 8 i .. 8 i + 7 of the 32-byte digest are digest[i], little-endian */
template <typename ByteAt>
KECCAK_FN void keccak_sponge256(const ByteAt &byte_at, size_t len, uint8_t pad, uint64_t digest[4]) {
    uint64_t a[25];
    a[0] = a[1] = a[2] = a[3] = a[4] = a[5] = a[6] = a[7] = a[8] = a[9] = a[10] = a[11] = a[12] = 0;
    a[13] = a[14] = a[15] = a[16] = a[17] = a[18] = a[19] = a[20] = a[21] = a[22] = a[23] = a[24] = 0;
    const size_t blocks = len / KECCAK_RATE + 1;
    const size_t last = blocks * KECCAK_RATE - 1;
    for (size_t blk = 0; blk < blocks; ++blk) {
        const size_t base = blk * KECCAK_RATE;
#define KECCAK_ABSORB(i) a[i] ^= keccak_lane(byte_at, len, pad, last, base + 8 * (i))
        KECCAK_ABSORB(0);
        KECCAK_ABSORB(1);
        KECCAK_ABSORB(2);
        KECCAK_ABSORB(3);
        KECCAK_ABSORB(4);
        KECCAK_ABSORB(5);
        KECCAK_ABSORB(6);
        KECCAK_ABSORB(7);
        KECCAK_ABSORB(8);
        KECCAK_ABSORB(9);
        KECCAK_ABSORB(10);
        KECCAK_ABSORB(11);
        KECCAK_ABSORB(12);
        KECCAK_ABSORB(13);
        KECCAK_ABSORB(14);
        KECCAK_ABSORB(15);
        KECCAK_ABSORB(16);
#undef KECCAK_ABSORB
        keccak_f1600(a);
    }
    digest[0] = a[0];
    digest[1] = a[1];
    digest[2] = a[2];
    digest[3] = a[3];
}

#endif /* MXX_KECCAK_H */
