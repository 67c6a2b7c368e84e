// layout.hip — the storage layout of a matrix: 4-byte words, or 3 bytes per residue (GPU_MATRIX_LAYOUT_PACKED24).
//
// Moduli below 2^24 leave the top byte of every 32-bit word zero.  A uniform sample - the large operand B of a skinny
// product, which that product streams exactly once - is stored packed: 3N bytes per (poly, limb) row, residue i
// little-endian at bytes [3i, 3i+3), rows in the order of the words layout.  The register-tile product reads it as
// it is (arith.hip); every other consumer reaches the storage through words_ptr(), which unpacks the matrix once, on
// its context's stream, and leaves it in words.  DESIGN.md section 6c.
#include "common.h"

#include <stdexcept>

namespace {

// 4 residues per lane: 12 bytes in, 16 out.  N % 4 == 0, so `groups` covers the matrix exactly and a lane's 12 bytes
// never straddle two rows (rows are 3N bytes, a multiple of 12).
__global__ void __launch_bounds__(256) unpack24_kernel(uint4 *__restrict__ words, const uint32_t *__restrict__ packed, size_t groups) {
    const size_t g = item_index();
    if (g >= groups) return;
    const uint32_t *p = packed + 3 * g;
    const uint32_t w0 = __builtin_nontemporal_load(p), w1 = __builtin_nontemporal_load(p + 1), w2 = __builtin_nontemporal_load(p + 2);
    words[g] = make_uint4(w0 & 0xffffffu, __builtin_amdgcn_alignbit(w1, w0, 24) & 0xffffffu,
                          __builtin_amdgcn_alignbit(w2, w1, 16) & 0xffffffu, w2 >> 8);
}

// the other direction, for the transforms without a packed store (ring sizes other than 2^14, path overrides)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) pack24_kernel(uint32_t *__restrict__ packed, const u32x4 *__restrict__ words, size_t groups) {
    const size_t g = item_index();
    if (g >= groups) return;
    const u32x4 w = __builtin_nontemporal_load(words + g);
    uint32_t *p = packed + 3 * g;
    p[0] = w.x | (w.y << 24);
    p[1] = (w.y >> 8) | (w.z << 16);
    p[2] = (w.z >> 16) | (w.w << 8);
}

// launches on m's context with its device current, the caller's device restored afterwards
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace

void *words_ptr(const GpuMatrix *cm) {
    if (cm->layout.v.load(std::memory_order_acquire) == GPU_MATRIX_LAYOUT_WORDS) return cm->storage;
    // inputs are const: several host threads may hold this matrix; the first one converts it, under the lock, and the
    // others find words.  Packed launches hold the same lock, so the packed block is never freed between another
    // thread's look-up and its launch.
    GpuMatrix *m = const_cast<GpuMatrix *>(cm);
    GpuContext *ctx = m->ctx;
    std::lock_guard<std::mutex> lk(ctx->layout_mutex);
    if (m->layout.v.load(std::memory_order_relaxed) == GPU_MATRIX_LAYOUT_WORDS) return m->storage;
    DeviceScope dev(ctx->device);
    void *words = nullptr;
    if (ctx_alloc(ctx, m->bytes, &words)) throw std::runtime_error("unpacking a packed matrix: device allocation failed");
    const size_t groups = m->bytes / 16;
    // not bracketed by the launch trace: words_ptr() is often evaluated among the arguments of a traced launch, and a
    // conversion happens once per matrix (its time then counts towards that launch)
    g_kernel_launches.fetch_add(1, std::memory_order_relaxed);
    hipLaunchKernelGGL(unpack24_kernel, item_grid(groups, 256), dim3(256), 0, ctx->stream, static_cast<uint4 *>(words),
                       static_cast<const uint32_t *>(m->storage), groups);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ctx_free(ctx, words);
        throw std::runtime_error(std::string("unpacking a packed matrix: ") + hipGetErrorString(e));
    }
    ctx_free(ctx, m->storage);  // stream-ordered: after the unpack and every packed read enqueued before it
    m->storage = words;
    m->layout.v.store(GPU_MATRIX_LAYOUT_WORDS, std::memory_order_release);
    return words;
}

const void *packed24_ptr(const GpuMatrix *m, bool *packed) {
    *packed = m->layout.v.load(std::memory_order_acquire) == GPU_MATRIX_LAYOUT_PACKED24;
    return m->storage;
}

bool pack24_eligible(const GpuMatrix *m) {
    return m->ctx->pack24_ok && m->ctx->env.pack24 && !m->borrowed && m->bytes > 0 &&
           m->layout.v.load(std::memory_order_acquire) == GPU_MATRIX_LAYOUT_WORDS;
}

int pack24_store(GpuMatrix *m, bool ntt) {
    GpuContext *ctx = m->ctx;
    const uint32_t L = static_cast<uint32_t>(matrix_limbs(m));
    const size_t vectors = matrix_polys(m) * L;
    std::unique_lock<std::mutex> lk(ctx->layout_mutex);
    if (m->views) {  // row views share the words: the matrix stays as it is
        lk.unlock();
        return ntt ? launch_ntt(ctx, m->storage, vectors, static_cast<int>(L), false) : 0;
    }
    CtxBlock packed(ctx);
    if (packed.alloc(packed24_bytes(m))) return 1;
    // out of place: packing in place would race (vector v's packed bytes overlap the words of vector 3v/4)
    int rc = ntt ? launch_ntt_fwd_pack24_u32(ctx, static_cast<uint32_t *>(packed.ptr), static_cast<const uint32_t *>(m->storage), vectors, L) : -1;
    if (rc < 0) {
        if (ntt && (rc = launch_ntt(ctx, m->storage, vectors, static_cast<int>(L), false))) return rc;
        const size_t groups = m->bytes / 16;
        MXX_TRACE_BYTES(static_cast<double>(packed24_bytes(m)) + m->bytes);
        MXX_LAUNCH(pack24_kernel, item_grid(groups, 256), dim3(256), 0, ctx->stream, static_cast<uint32_t *>(packed.ptr),
                   static_cast<const u32x4 *>(m->storage), groups);
        HIP_TRY(hipGetLastError());
    } else if (rc) {
        return rc;
    }
    ctx_free(ctx, m->storage);  // stream-ordered, behind the kernel that read it
    m->storage = packed.release();
    m->layout.v.store(GPU_MATRIX_LAYOUT_PACKED24, std::memory_order_release);
    return 0;
}
