// hash_seed.hip — tags to sampler seeds on the device.
// hash_seed_for_matrix of the reference (src/sampler/gpu.rs:118-136) is
//     seed = H("GpuDCRTPolyHashSampler/v2" || key || tag || counter_le32)
// with H = Keccak-256 wherever the reference instantiates it; the digest is 32 bytes, a seed is 32 bytes, so the
// reference's counter loop runs once, with counter 0.  The tagged loops of src/commit/wee25.rs:687-703,858-883,
// src/lookup/ggh15/pubkey_gpu.rs:398-401,924,1296 and src/lookup/lwe/pubkey_gpu.rs:559,616 hash one tag per index on
// the host and upload the seeds; here one lane hashes one tag (keccak.h: the state in registers, the message never laid
// out in memory) and the seeds stay where the block sampler reads them (sampling.hip, sample_blocks_impl).
//
// One lane per tag and not a wave per tag: Keccak-f is 25 lanes of 64 bits mixed across both axes in every round, so a
// cooperative form pays cross-lane traffic in each of the 24 rounds for a message that is one rate block (two for tags
// past 74 bytes); the callers' counts (tens to 2^20 tags) fill the chip with independent sponges or are too small for
// the launch to matter either way.
#include "common.h"
#include "keccak.h"

#include <cstring>

static constexpr size_t kMaxTags = size_t(1) << 20;
static constexpr uint32_t kPrefixLen = 25;  // "GpuDCRTPolyHashSampler/v2"
static constexpr uint32_t kKeyLen = 32;
static constexpr uint32_t kMaxIndexedPrefix = 64;
__constant__ const char kDomain[kPrefixLen + 1] = "GpuDCRTPolyHashSampler/v2";

// where lane t's tag comes from; passed by value in the kernel arguments
struct HashTagSource {
    int form;                 // GPUPOLY_TAGS_*
    uint32_t prefix_len;      // INDEXED
    uint64_t first_index;     // INDEXED: tag t = prefix || encoding of first_index + t
    const uint8_t *bytes;     // TABLE: tag t = bytes[offsets[t] .. offsets[t + 1])
    const uint64_t *offsets;  // TABLE: ntags + 1 of them
    uint64_t prefix[kMaxIndexedPrefix / 8];  // INDEXED: the prefix, little-endian in words
};
struct HashKey {
    uint64_t words[kKeyLen / 8];  // the 32 key bytes, little-endian in words
};

__device__ __forceinline__ uint8_t byte_of_words(const uint64_t *words, uint32_t j) {
    return static_cast<uint8_t>(words[j >> 3] >> (8 * (j & 7)));
}

// byte `pos` of prefix25 || key || tag || 00 00 00 00 for one tag
struct SeedMessage {
    const HashKey &key;
    const HashTagSource &src;
    const uint8_t *tag_bytes;  // TABLE: this tag's first byte
    uint32_t tag_len;
    uint64_t index;            // INDEXED: first_index + t
    uint64_t digits_lo;        // INDEXED_DECIMAL: decimal digit j of index (0 = units) in nibble j; digits 16..19 in digits_hi
    uint32_t digits_hi, ndigits;

    __device__ __forceinline__ uint8_t tag_byte(uint32_t j) const {
        if (src.form == GPUPOLY_TAGS_TABLE) return tag_bytes[j];
        if (j < src.prefix_len) return byte_of_words(src.prefix, j);
        const uint32_t k = j - src.prefix_len;
        if (src.form == GPUPOLY_TAGS_INDEXED_LE64) return static_cast<uint8_t>(index >> (8 * k));
        const uint32_t d = ndigits - 1 - k;  // most significant digit first
        const uint32_t nib = d < 16 ? static_cast<uint32_t>(digits_lo >> (4 * d)) : digits_hi >> (4 * (d - 16));
        return static_cast<uint8_t>('0' + (nib & 15u));
    }
    __device__ __forceinline__ uint8_t operator()(size_t pos) const {
        const uint32_t p = static_cast<uint32_t>(pos);
        if (p < kPrefixLen) return static_cast<uint8_t>(kDomain[p]);
        if (p < kPrefixLen + kKeyLen) return byte_of_words(key.words, p - kPrefixLen);
        if (p < kPrefixLen + kKeyLen + tag_len) return tag_byte(p - kPrefixLen - kKeyLen);
        return 0;  // the counter: 0 as four little-endian bytes
    }
};

// the seed of tag t
__device__ __forceinline__ GpuRngSeed seed_of_tag(const HashKey &key, const HashTagSource &src, size_t t, uint8_t pad) {
    SeedMessage msg{key, src, nullptr, 0, 0, 0, 0, 0};
    if (src.form == GPUPOLY_TAGS_TABLE) {
        const uint64_t lo = src.offsets[t], hi = src.offsets[t + 1];
        msg.tag_bytes = src.bytes + lo;
        msg.tag_len = static_cast<uint32_t>(hi - lo);
    } else {
        msg.index = src.first_index + t;
        if (src.form == GPUPOLY_TAGS_INDEXED_LE64) {
            msg.tag_len = src.prefix_len + 8;
        } else {
            uint64_t v = msg.index;
            uint32_t n = 1;
#pragma unroll
            for (uint32_t d = 0; d < 20; ++d) {  // 2^64 - 1 has 20 digits
                const uint64_t q = v / 10u, r = v - q * 10u;
                if (d < 16) msg.digits_lo |= r << (4 * d);
                else msg.digits_hi |= static_cast<uint32_t>(r) << (4 * (d - 16));
                if (v != 0) n = d + 1;
                v = q;
            }
            msg.ndigits = n;
            msg.tag_len = src.prefix_len + n;
        }
    }
    uint64_t digest[4];
    keccak_sponge256(msg, static_cast<size_t>(kPrefixLen + kKeyLen + 4) + msg.tag_len, pad, digest);
    // the digest's bytes as GpuRngSeed::from_bytes reads them: four little-endian words
    GpuRngSeed seed;
    seed.words[0] = digest[0];
    seed.words[1] = digest[1];
    seed.words[2] = digest[2];
    seed.words[3] = digest[3];
    return seed;
}

// one lane per tag, grid-stride
__global__ void __launch_bounds__(256) hash_seeds_kernel(GpuRngSeed *__restrict__ seeds, size_t ntags, HashKey key, HashTagSource src, uint32_t pad) {
    const size_t stride = static_cast<size_t>(gridDim.x) * gridDim.y * blockDim.x;
    for (size_t t = item_index(); t < ntags; t += stride) seeds[t] = seed_of_tag(key, src, t, static_cast<uint8_t>(pad));
}

// ---- host side ----------------------------------------------------------------------------------------------------
int hash_tags_check(const char *entry, const GpuHashTags *tags, size_t ntags, size_t *table_bytes) {
    const auto refuse = [entry](const char *what) { return set_error(std::string(entry) + what); };
    *table_bytes = 0;
    if (!tags) return refuse(": null tags");
    if (tags->hash != GPUPOLY_HASH_KECCAK256 && tags->hash != GPUPOLY_HASH_SHA3_256) return refuse(": unknown hash");
    if (tags->form == GPUPOLY_TAGS_TABLE) {
        const size_t *off = tags->tag_offsets;
        if (!off) return refuse(": the table form needs tag_offsets");
        if (off[0] != 0) return refuse(": tag_offsets must start at 0");
        for (size_t t = 0; t < ntags; ++t) {
            if (off[t + 1] < off[t]) return refuse(": tag_offsets must not decrease");
            if ((off[t + 1] - off[t]) >> 31) return refuse(": a tag of 2^31 bytes or more");
        }
        if (off[ntags] && !tags->tags) return refuse(": null tag bytes for tags that are not all empty");
        *table_bytes = off[ntags];
    } else if (tags->form == GPUPOLY_TAGS_INDEXED_LE64 || tags->form == GPUPOLY_TAGS_INDEXED_DECIMAL) {
        if (tags->tag_offsets) return refuse(": the indexed forms take no tag_offsets");
        if (tags->prefix_len > kMaxIndexedPrefix) return refuse(": prefix_len above 64");
        if (tags->prefix_len && !tags->tags) return refuse(": null prefix");
        if (ntags && tags->first_index > ~uint64_t(0) - (ntags - 1)) return refuse(": the index range wraps");
    } else {
        return refuse(": unknown tag form");
    }
    return 0;
}

size_t hash_tags_staged_words(const GpuHashTags *tags, size_t ntags, size_t table_bytes) {
    return tags->form == GPUPOLY_TAGS_TABLE ? ntags + 1 + (table_bytes + 7) / 8 : 0;
}

void hash_tags_stage(const GpuHashTags *tags, size_t ntags, size_t table_bytes, uint64_t *staging) {
    if (tags->form != GPUPOLY_TAGS_TABLE) return;
    for (size_t t = 0; t <= ntags; ++t) staging[t] = tags->tag_offsets[t];
    if (table_bytes) {
        staging[ntags + (table_bytes + 7) / 8] = 0;  // the last word's tail
        std::memcpy(staging + ntags + 1, tags->tags, table_bytes);
    }
}

int launch_hash_seeds(GpuContext *ctx, GpuRngSeed *d_seeds, const GpuHashTags *tags, size_t ntags, const uint64_t *d_staged) {
    HashTagSource src{};
    src.form = tags->form;
    if (tags->form == GPUPOLY_TAGS_TABLE) {
        src.offsets = d_staged;
        src.bytes = reinterpret_cast<const uint8_t *>(d_staged + ntags + 1);
    } else {
        src.prefix_len = static_cast<uint32_t>(tags->prefix_len);
        src.first_index = tags->first_index;
        if (tags->prefix_len) std::memcpy(src.prefix, tags->tags, tags->prefix_len);
    }
    HashKey key;
    std::memcpy(key.words, tags->key, kKeyLen);
    const uint32_t pad = tags->hash == GPUPOLY_HASH_SHA3_256 ? KECCAK_PAD_SHA3_256 : KECCAK_PAD_KECCAK256;
    const size_t blocks = (ntags + 255) / 256;
    MXX_LAUNCH(hash_seeds_kernel, dim3(static_cast<unsigned>(blocks < 1024 ? blocks : 1024)), dim3(256), 0, ctx->stream, d_seeds, ntags, key, src, pad);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int gpupoly_hash_seeds(GpuContext *ctx, const GpuHashTags *tags, size_t ntags, GpuRngSeed *seeds_out) {
    ABI_GUARD_BEGIN
    static const char *const entry = "gpupoly_hash_seeds";
    if (!ctx) return set_error("gpupoly_hash_seeds: null context");
    if (!seeds_out) return set_error("gpupoly_hash_seeds: null seeds_out");
    if (ntags == 0 || ntags > kMaxTags) return set_error("gpupoly_hash_seeds: the tag count must be 1..2^20");
    size_t table_bytes = 0;
    if (hash_tags_check(entry, tags, ntags, &table_bytes)) return 1;
    if (ctx_activate(ctx)) return 1;
    const size_t staged = hash_tags_staged_words(tags, ntags, table_bytes);
    CtxBlock block(ctx);
    if (block.alloc(sizeof(GpuRngSeed) * ntags + sizeof(uint64_t) * staged)) return 1;
    GpuRngSeed *d_seeds = static_cast<GpuRngSeed *>(block.ptr);
    uint64_t *d_staged = reinterpret_cast<uint64_t *>(d_seeds + ntags);
    static thread_local std::vector<uint64_t> staging;
    if (staged) {
        staging.resize(staged);
        hash_tags_stage(tags, ntags, table_bytes, staging.data());
        MXX_TRACED_COPY("tag table (host to device)", ctx->stream, sizeof(uint64_t) * staged,
                        HIP_TRY(hipMemcpyAsync(d_staged, staging.data(), sizeof(uint64_t) * staged, hipMemcpyHostToDevice, ctx->stream)));
    }
    if (launch_hash_seeds(ctx, d_seeds, tags, ntags, d_staged)) return 1;
    HIP_TRY(hipMemcpyAsync(seeds_out, d_seeds, sizeof(GpuRngSeed) * ntags, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
    ABI_GUARD_END
}
