// matmul_skinny24.hip — the one-row product against a PACKED24 right operand: C (1 x cols) = A (1 x inner) * B (inner x cols),
// 32-bit words, A in words, B at 3 bytes per residue (layout.hip), streamed exactly once with non-temporal loads.
//
// The same grid, the same products and the same reductions as matmul_kernel<u32,1,TC,4,nt,packed24 B> (arith.hip), so
// results are bit-identical; what differs is how B reaches the lanes and in what order (DESIGN.md 6c,
// profiles/skinny24_notes.md):
//   TC   columns per lane (8 or 4), 4 slots each
//   G    columns whose loads are issued together before their unpack and MACs: G = TC is matmul_kernel's burst of TC
//        requests per inner step, G = 1 the words kernel's one request at a time
//   WPE  waves per SIMD the register allocation is held to (__launch_bounds__)
//   MAP  12: a lane loads its own 12 bytes (dwordx3; a 16-lane group is 192 bytes, so groups 1 and 3 of a wave start in
//        the middle of a 128-byte line).  16: lanes 0..47 load 16 bytes each (a 16-lane group is two whole lines), the wave
//        parks its 768-byte run in a slice of LDS of its own and every lane reads its 12 bytes back.  Needs whole waves:
//        N % 256 == 0; other rings run MAP = 12.
// Column bases are wave-uniform (blockIdx and kernel arguments only) and the lane adds one 32-bit byte offset.  The loads
// are buffer loads (a descriptor of one row in scalar registers + that offset): written as `uniform pointer + lane offset`
// the compiler widens the offset once outside the loop and forms 64-bit vector addresses per load again.  A descriptor
// spans one inner step of B - every column's row of one k - and the column is a scalar offset into it.
#include "common.h"
#include "matmul_tile.h"
#include "modarith.h"

#include <map>
#include <string>

namespace skinny24 {

typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// `bytes` bytes at the wave-uniform `base` as a raw buffer (gfx9 family: 32-bit data format, no swizzle)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const char *base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(base), 0, static_cast<int>(bytes), 0x00020000);
}
constexpr int kAuxNT = 2;  // the buffer loads' non-temporal bit

__device__ __forceinline__ void unpack4(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t *o) {
    o[0] = w0 & 0xffffffu;
    o[1] = __builtin_amdgcn_alignbit(w1, w0, 24) & 0xffffffu;
    o[2] = __builtin_amdgcn_alignbit(w2, w1, 16) & 0xffffffu;
    o[3] = w2 >> 8;
}

template <int TC, int G, int WPE, int MAP>
__global__ void __launch_bounds__(256, WPE)
    kernel(uint32_t *__restrict__ C, const uint32_t *__restrict__ A, const uint32_t *__restrict__ B, const LimbConst *__restrict__ limbs,
           uint32_t inner, uint32_t cols, uint32_t L, uint32_t N) {
    static_assert((TC == 8 || TC == 4) && TC % G == 0 && (MAP == 12 || MAP == 16), "skinny24 shape");
    const uint32_t limb = blockIdx.z, c0 = blockIdx.y * TC;
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) * 4;  // the lane's first slot
    if (i >= N) return;  // MAP == 16 runs whole waves only (the launcher)
    const LimbConst lc = limbs[limb];
    const uint32_t q = static_cast<uint32_t>(lc.q);

    // wave-uniform bases in bytes; columns past the edge are clamped to the last one and their results dropped
    uint32_t bcol[TC];  // within one inner step of B: `bstep` bytes, below 2^32 (the launcher)
#pragma unroll
    for (int c = 0; c < TC; ++c) bcol[c] = ((min(c0 + c, cols - 1)) * L + limb) * N * 3;
    const uint32_t bstep = cols * L * N * 3;
    const char *bk = reinterpret_cast<const char *>(B);
    const char *arow = reinterpret_cast<const char *>(A) + static_cast<size_t>(limb) * N * 4;
    const size_t astep = static_cast<size_t>(L) * N * 4;
    const uint32_t a_off = i * 4;
    const uint32_t lane = threadIdx.x & 63u;
    // MAP 12: the lane's own 12 bytes; MAP 16: 16 bytes of the wave's 768-byte run in lanes 0..47, and the offset just past a
    // step of B in lanes 48..63, which the descriptor's range check answers with zeros and no request
    const uint32_t b_off = MAP == 12 ? i * 3 : (lane < 48 ? (i - lane * 4) * 3 + lane * 16 : bstep);
    __shared__ u32x4 stage[MAP == 16 ? 4 : 1][MAP == 16 ? G : 1][64];  // per wave and column 48 entries of data, 16 never read
    const uint32_t wave = threadIdx.x >> 6;

    uint64_t acc[TC][4];
#pragma unroll
    for (int c = 0; c < TC; ++c)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[c][s] = 0;
    const uint32_t lazy = lc.lazy_terms;
    uint32_t pending = 0;
    for (uint32_t k = 0; k < inner; ++k) {
        const u32x4 av = __builtin_amdgcn_raw_buffer_load_b128(row_rsrc(arow, N * 4), a_off, 0, 0);
        arow += astep;
#pragma unroll
        for (int g0 = 0; g0 < TC; g0 += G) {  // per group: load, then unpack, then multiply
            uint32_t raw[G][3];
            if constexpr (MAP == 12) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const u32x3 t = __builtin_amdgcn_raw_buffer_load_b96(row_rsrc(bk, bstep), b_off, bcol[g0 + g], kAuxNT);
                    raw[g][0] = t[0];
                    raw[g][1] = t[1];
                    raw[g][2] = t[2];
                }
            } else {
                // the wave's own slice: LDS serves a wave's accesses in order, so the wave needs no barrier, only the
                // compiler must keep the order (the two wave barriers emit no instruction)
                __builtin_amdgcn_wave_barrier();
                u32x4 t[G];
#pragma unroll
                for (int g = 0; g < G; ++g) t[g] = __builtin_amdgcn_raw_buffer_load_b128(row_rsrc(bk, bstep), b_off, bcol[g0 + g], kAuxNT);
#pragma unroll
                for (int g = 0; g < G; ++g) stage[wave][g][lane] = t[g];
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const uint32_t *p = reinterpret_cast<const uint32_t *>(&stage[wave][g][0]) + lane * 3;
                    raw[g][0] = p[0];
                    raw[g][1] = p[1];
                    raw[g][2] = p[2];
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                uint32_t bv[4];
                unpack4(raw[g][0], raw[g][1], raw[g][2], bv);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[g0 + g][s] += static_cast<uint64_t>(av[s]) * static_cast<uint64_t>(bv[s]);
            }
        }
        bk += bstep;
        if (++pending == lazy) {
            pending = 0;
#pragma unroll
            for (int c = 0; c < TC; ++c)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[c][s] = reduce_u64_sum(acc[c][s], q, lc.mu64);
        }
    }
#pragma unroll
    for (int c = 0; c < TC; ++c) {
        if (c0 + c >= cols) continue;
        u32x4 o;
#pragma unroll
        for (int s = 0; s < 4; ++s) o[s] = reduce_u64_sum(acc[c][s], q, lc.mu64);
        *reinterpret_cast<u32x4 *>(C + (static_cast<size_t>(c0 + c) * L + limb) * N + i) = o;
    }
}

// the instantiated shapes: X(TC, G, WPE, MAP), each without spills and within the registers of its WPE.  Eight columns at six
// waves per SIMD (80 registers: 64 of accumulators, the operands, and the final reductions' temporaries) spill two registers
// already at G = 1 and 2 and are left out; more waves than five come with four columns.  Their MAP 12 loads the compiler issues four at a
// time whatever G says: 4,1,8,12 and 4,2,8,12 are the loop of 4,4,8,12 and stay as what their MAP 16 forms fall back to on a
// ring of partial waves.  MAP 16 with G = 8 would need all of a CU's LDS.
#define MXX_SKINNY24_SHAPES(X)                                          \
    X(8, 1, 5, 12) X(8, 2, 5, 12) X(8, 4, 5, 12) X(8, 8, 5, 12) X(8, 8, 4, 12)  \
    X(8, 1, 5, 16) X(8, 2, 5, 16) X(8, 4, 5, 16)                        \
    X(4, 1, 8, 12) X(4, 2, 8, 12) X(4, 4, 8, 12) X(4, 1, 8, 16) X(4, 2, 8, 16) X(4, 4, 8, 16)

constexpr int shape_key(int tc, int g, int wpe, int map) { return ((tc * 16 + g) * 16 + wpe) * 32 + map; }

}  // namespace skinny24

// EnvSwitches::skinny24_shape for MXX_HIP_SKINNY24=force:TC,G,WPE,MAP (0: not a shape)
int skinny24_parse_shape(const char *s) {
    int v[4] = {0, 0, 0, 0};
    for (int f = 0; f < 4; ++f) {
        if (*s < '0' || *s > '9') return 0;
        while (*s >= '0' && *s <= '9' && v[f] < 100) v[f] = v[f] * 10 + (*s++ - '0');
        if (f < 3 && *s++ != ',') return 0;
    }
    if (*s || v[0] > 15 || v[1] > 15 || v[2] > 15 || v[3] > 31) return 0;
    return skinny24::shape_key(v[0], v[1], v[2], v[3]);
}

// the shape the dispatcher takes by itself: the winner of the sweep at the M2A shape (profiles/skinny24_notes.md)
static constexpr int kSkinny24Default = skinny24::shape_key(8, 2, 5, 12);

// -1: not this kernel's product (the caller goes on to matmul_kernel); `small_grid`: the caller's loads-ahead case
int launch_matmul_skinny24(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs, bool small_grid) {
    using namespace skinny24;
    GpuContext *ctx = out->ctx;
    const EnvSwitches &env = ctx->env;
    if (env.skinny24 == 1 || ctx->wide || lhs->ctx != ctx || rhs->ctx != ctx) return -1;
    const uint32_t inner = static_cast<uint32_t>(lhs->cols), cols = static_cast<uint32_t>(rhs->cols);
    const uint32_t L = static_cast<uint32_t>(matrix_limbs(out)), N = static_cast<uint32_t>(ctx->N);
    if (lhs->rows != 1 || cols < 8 || N < 4) return -1;
    // the kernel's descriptor spans one inner step of B and its column offsets are 32-bit (16 bytes of margin: MAP 16's idle lanes)
    if (static_cast<uint64_t>(cols) * L * N * 3 >= 0xfffffff0ull) return -1;
    if (rhs->layout.v.load(std::memory_order_acquire) != GPU_MATRIX_LAYOUT_PACKED24) return -1;
    const bool force = env.skinny24 == 2;
    int key = force && env.skinny24_shape ? env.skinny24_shape : kSkinny24Default;
    const int tc = key / (16 * 16 * 32);
    const TileGrid g = tc == 4 ? tile_grid<1, 4, 4>(ctx, 1, cols, L, rhs->bytes) : tile_grid<1, 8, 4>(ctx, 1, cols, L, rhs->bytes);
    if (!force && (!g.streamed || small_grid)) return -1;
    if (!tile_grid_fits(1, cols, 1, tc == 4 ? 4 : 8)) return set_error("gpu_matrix_mul: matrix too large");
    const bool fell_back = key % 32 == 16 && N % 256 != 0;  // partial waves: every lane loads its own 12 bytes
    if (fell_back) key = key - 16 + 12;
    uint32_t *c = static_cast<uint32_t *>(words_ptr(out));  // before the layout lock below: it may unpack
    // one packed operand per product, as in launch_matmul_cfg: A is the small one and is read in words
    if (lhs->layout.v.load(std::memory_order_acquire) == GPU_MATRIX_LAYOUT_PACKED24) (void)words_ptr(lhs);
    std::lock_guard<std::mutex> lk(ctx->layout_mutex);
    bool pa = false, pb = false;
    const uint32_t *a = static_cast<const uint32_t *>(packed24_ptr(lhs, &pa)), *b = static_cast<const uint32_t *>(packed24_ptr(rhs, &pb));
    if (pa || !pb) return -1;  // another thread changed a layout since the look above
    const char *label;
    {
        static std::mutex label_mutex;
        static std::map<int, std::string> labels;  // node-based: a label's c_str() stays where it is
        std::lock_guard<std::mutex> ll(label_mutex);
        std::string &s = labels[key * 2 + (fell_back ? 1 : 0)];
        if (s.empty())
            s = "skinny24::kernel<TC=" + std::to_string(tc) + ",G=" + std::to_string(key / (16 * 32) % 16) + ",WPE=" + std::to_string(key / 32 % 16) +
                ",MAP=" + std::to_string(key % 32) + (fell_back ? " (16 asked: partial wave)" : "") +
                ",nt,packed24 B> (the tile of matmul_kernel<u32,1," + std::to_string(tc) + ",4,nt,packed24 B>, one row x TC columns x 4 slots per lane, " +
                "B streamed once with non-temporal loads, 3-byte residues, " +
                (key % 32 == 16 ? "16-byte requests through a wave-private LDS slice" : "12 bytes per lane") + ")";
        label = s.c_str();
    }
    switch (key) {
#define MXX_SKINNY24_CASE(TC_, G_, WPE_, MAP_)                                                                                               \
    case shape_key(TC_, G_, WPE_, MAP_):                                                                                                     \
        MXX_LAUNCH((kernel<TC_, G_, WPE_, MAP_>), g.grid, dim3(g.threads), 0, ctx->stream, c, a, b, ctx->d_limbs, inner, cols, L, N); \
        break;
        MXX_SKINNY24_SHAPES(MXX_SKINNY24_CASE)
#undef MXX_SKINNY24_CASE
        default: return set_error("gpu_matrix_mul: MXX_HIP_SKINNY24 names a shape that is not instantiated");
    }
    ctx->last_kernel = label;
    HIP_TRY(hipGetLastError());
    return 0;
}
