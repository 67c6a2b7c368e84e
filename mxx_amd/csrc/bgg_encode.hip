// bgg_encode.hip — the BGG+ encodings of P inputs in S slots in one call: gpupoly_matrix_bgg_encode_slots (DESIGN.md
// section 5za).
//
// BGGPolyEncodingSampler::sample (src/bgg/sampler.rs:224-364; on the device src/bgg/sampler_gpu.rs:81-172) is a plain loop
// over the slots that per slot (src/bgg/sampler_gpu.rs:110-160) loads the slot's secret mask from compact bytes, forms
// t = s S_slot, samples a fresh Gaussian 1 x P m error, builds the plaintext row, multiplies t A_all, multiplies t G against a
// filled gadget, takes the tensor product with the plaintexts, subtracts, adds, and slices the row into P vectors.
// BGGEncodingSampler::sample (src/bgg/sampler.rs:133-182) is the same with one slot and t = s.  With d the secret size,
// k = dpt L, m = d k and T the S x d matrix whose row sigma is t_sigma,
//
//   outs[i][sigma, c] = sum_j T[sigma, j] A_i[j, c]  -  pt[sigma][i] o T[sigma, c / k] w(c)  +  E[sigma, i m + c],   pt[.][0] = 1,
//
// w(c) = (2^base_bits)^e in limb tower(c) and 0 in every other limb (c = (c / k) k + tower(c) dpt + e), E row sigma the
// 1 x P m Gaussian sample under seeds[sigma].  Everything is exact arithmetic on canonical residues, so one lazy sum per
// output word - the error residue first, the d products, the gadget term in the one limb that has it - equals the
// reference's sequence bit for bit.  Per group of slots: the stacked Gaussian block sample into scratch, ONE staged copy of
// the table (output and public-key pointers, the gadget weights) and ONE kernel.  No G, no tensor product, no temporaries,
// nothing launched per slot or per input.
#include "common.h"
#include "modarith.h"
#include "row_targets.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace {

// the group's device table: [P] output pointers, [P] public-key pointers, [L][dpt] gadget weights
struct BggEncodeArgs {
    const void *secrets;     // S x d
    const void *plaintexts;  // S x (P - 1), null when P == 1
    const void *errors;      // S x (P m), null: no error
    const uint64_t *table;
    size_t m, k, entries;
    uint32_t S, P, d, L, dpt, logN, slot_tiles;
};

// A block's tile: slots [s0, s0 + TS) x column c of input i in limb l (blockIdx.y/z, the slot tile fastest so that the
// tiles that read the same d words of A_i[., c] are neighbours), blockIdx.x strides the limb vector's N words VN per lane
// (16 bytes, or one word where a limb vector is narrower).  Input, column, limb and with them the gadget's hit, its digit
// and its weight are uniform per block.  A lane loads the d words of A_i[., c] once for the tile's TS slots; slots past the
// end repeat the last one and are never stored.  The TS x VN sums share one count of pending terms - LazyAcc's rule
// (row_targets.h) with the count kept once; they start at the error's residue, or 0.
template <typename W, int VN, int TS>
__global__ void __launch_bounds__(256) bgg_encode_kernel(BggEncodeArgs a, const LimbConst *__restrict__ limbs) {
    typedef typename CombineVec<W, VN>::V V;
    typedef typename Wide<W>::type D;
    const size_t entry = static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y;
    if (entry >= a.entries) return;
    const size_t poly = entry / a.slot_tiles;
    const uint32_t st = static_cast<uint32_t>(entry - poly * a.slot_tiles);
    const size_t pc = poly / a.L;
    const uint32_t l = static_cast<uint32_t>(poly - pc * a.L);
    const size_t i = pc / a.m, c = pc - i * a.m;
    const size_t jb = c / a.k;
    const uint32_t loc = static_cast<uint32_t>(c - jb * a.k), tw = loc / a.dpt, e = loc - tw * a.dpt;
    const bool hit = tw == l;
    const LimbConst lc = limbs[l];
    const uint32_t lazy = lc.lazy_terms;
    const W q = static_cast<W>(lc.q);
    const W weight = static_cast<W>(a.table[2 * static_cast<size_t>(a.P) + static_cast<size_t>(l) * a.dpt + e]);
    const size_t wpp = static_cast<size_t>(a.L) << a.logN, n = size_t(1) << a.logN, lo = static_cast<size_t>(l) << a.logN;
    W *out = reinterpret_cast<W *>(a.table[i]);
    const W *A = reinterpret_cast<const W *>(a.table[a.P + i]) + c * wpp + lo;
    const W *T = static_cast<const W *>(a.secrets) + lo;
    const W *E = a.errors ? static_cast<const W *>(a.errors) + (i * a.m + c) * wpp + lo : nullptr;
    const W *pt = i ? static_cast<const W *>(a.plaintexts) + (i - 1) * wpp + lo : nullptr;
    const size_t e_cols = static_cast<size_t>(a.P) * a.m, pt_cols = a.P - 1;
    size_t slot[TS];
#pragma unroll
    for (int s = 0; s < TS; ++s) slot[s] = min(static_cast<size_t>(st) * TS + s, static_cast<size_t>(a.S) - 1);
    for (size_t x0 = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * VN; x0 < n; x0 += static_cast<size_t>(gridDim.x) * blockDim.x * VN) {
        D acc[TS][VN];
        uint32_t pending = 0;
#pragma unroll
        for (int s = 0; s < TS; ++s) {
            W ev[VN];
            if (E) *reinterpret_cast<V *>(ev) = *reinterpret_cast<const V *>(E + slot[s] * e_cols * wpp + x0);
#pragma unroll
            for (int x = 0; x < VN; ++x) acc[s][x] = E ? ev[x] : W(0);
        }
        auto fold = [&]() {
#pragma unroll
            for (int s = 0; s < TS; ++s)
#pragma unroll
                for (int x = 0; x < VN; ++x) acc[s][x] = lazy_reduce<W>(acc[s][x], lc);
            pending = 0;
        };
        for (size_t j = 0; j < a.d; ++j) {
            W av[VN], tv[TS][VN];
            *reinterpret_cast<V *>(av) = *reinterpret_cast<const V *>(A + j * a.m * wpp + x0);
#pragma unroll
            for (int s = 0; s < TS; ++s) *reinterpret_cast<V *>(tv[s]) = *reinterpret_cast<const V *>(T + (slot[s] * a.d + j) * wpp + x0);
            if (pending >= lazy) fold();
#pragma unroll
            for (int s = 0; s < TS; ++s)
#pragma unroll
                for (int x = 0; x < VN; ++x) acc[s][x] += static_cast<D>(tv[s][x]) * av[x];
            ++pending;
        }
        if (hit) {  // - pt o t w as one more term: (q - pt t mod q) w, the negation canonical so that the term stays below (q - 1)^2
            W gv[TS][VN];
#pragma unroll
            for (int s = 0; s < TS; ++s) {
                *reinterpret_cast<V *>(gv[s]) = *reinterpret_cast<const V *>(T + (slot[s] * a.d + jb) * wpp + x0);
                if (pt) {
                    W pv[VN];
                    *reinterpret_cast<V *>(pv) = *reinterpret_cast<const V *>(pt + slot[s] * pt_cols * wpp + x0);
#pragma unroll
                    for (int x = 0; x < VN; ++x) gv[s][x] = mul_mod<W>(pv[x], gv[s][x], q, lc.mu, lc.kbits);
                }
            }
            if (pending >= lazy) fold();
#pragma unroll
            for (int s = 0; s < TS; ++s)
#pragma unroll
                for (int x = 0; x < VN; ++x) acc[s][x] += static_cast<D>(gv[s][x] ? static_cast<W>(q - gv[s][x]) : W(0)) * weight;
            ++pending;
        }
#pragma unroll
        for (int s = 0; s < TS; ++s) {
            if (static_cast<size_t>(st) * TS + s >= a.S) continue;
            W o[VN];
#pragma unroll
            for (int x = 0; x < VN; ++x) o[x] = lazy_reduce<W>(acc[s][x], lc);
            *reinterpret_cast<V *>(out + (slot[s] * a.m + c) * wpp + lo + x0) = *reinterpret_cast<const V *>(o);
        }
    }
}

// what one accepted call works with: S slots, P inputs, secrets S x d, public keys d x m, m = d k
struct BggEncodeCall : RowCall {
    size_t S, P, d, m;
    size_t cap;  // a group's scratch
};

inline std::string input_at(size_t i) { return " (input " + std::to_string(i) + ")"; }

int slot_tile(size_t S) { return S >= 3 ? 4 : S == 2 ? 2 : 1; }
size_t tile_entries(const BggEncodeCall &call, size_t Sg) {
    const size_t ts = slot_tile(Sg);
    return call.P * call.m * call.L * ((Sg + ts - 1) / ts);
}

// Everything both entries refuse, for every input, before anything is launched.  `samples`: the sampling entry, whose sigma
// and seeds are checked; otherwise the combine entry with the errors given or null.  (*go): something is left to launch
int check_call(const char *who, GpuMatrix *const *outs, size_t P, const GpuMatrix *secrets, const GpuMatrix *const *pubkeys,
               const GpuMatrix *plaintexts, uint32_t base_bits, bool samples, double sigma, const GpuRngSeed *seeds, const GpuMatrix *errors,
               BggEncodeCall *call) {
    const Refuse refuse{who};
    if (!outs || !pubkeys) return refuse("null array");
    if (!secrets) return refuse("null secrets");
    if (int rc = refuse_null_outputs(refuse, outs, P, [](size_t i) { return "null output" + input_at(i); })) return rc;
    for (size_t i = 0; i < P; ++i)
        if (!pubkeys[i]) return refuse("null public key" + input_at(i));
    if (P > 1 && !plaintexts) return refuse("null plaintexts: inputs 1.. bring a plaintext each");
    if (P == 1 && plaintexts) return refuse("plaintexts given with one input: input 0's plaintext is the constant 1");
    if (samples && !(sigma >= 0.0 && std::isfinite(sigma))) return refuse("sigma must be finite and not negative");
    const bool draws = samples && sigma > 0.0;
    if (draws && !seeds) return refuse("null seeds");
    if (int rc = refuse_base_level(refuse, secrets, base_bits, false, call)) return rc;
    GpuContext *ctx = call->ctx;
    const size_t S = secrets->rows, d = secrets->cols, m = d * call->k;
    if (S > (size_t(1) << 20)) return refuse("at most 2^20 slots");
    if (secrets->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format (secrets)");
    if (P > 0xffffffffull || d > 0xffffffffull || m > 0xffffffffull) return refuse("matrix too large");
    for (size_t i = 0; i < P; ++i) {
        const std::string at = input_at(i);
        if (int rc = refuse_foreign(refuse, pubkeys[i], *call, at)) return rc;
        if (pubkeys[i]->rows != d) return refuse("shape mismatch: a public key has one row per secret column" + at);
        if (pubkeys[i]->cols != m) return refuse("shape mismatch: a public key is d x m, m = d * digits per tower * limbs" + at);
        if (pubkeys[i]->format != GPU_POLY_FORMAT_EVAL) return refuse("requires Eval format" + at);
    }
    if (plaintexts)
        if (int rc = refuse_operand(refuse, plaintexts, *call, S, P - 1, "shape mismatch: the plaintexts are slots x (inputs - 1)")) return rc;
    if (errors)
        if (int rc = refuse_operand(refuse, errors, *call, S, P * m, "shape mismatch: the errors are slots x (inputs * m)")) return rc;
    if (int rc = refuse_outputs(refuse, outs, P, *call, input_at, [&](const GpuMatrix *out) -> const char * {
            return out->rows != S || out->cols != m ? "shape mismatch: an output is slots x m" : nullptr;
        }))
        return rc;
    call->S = S, call->P = P, call->d = d, call->m = m;
    call->cap = ctx->env.bgg_encode_budget ? ctx->env.bgg_encode_budget : kRowGroupBytes;
    // an output is written while every operand is still being read, and by no other input
    std::vector<const GpuMatrix *> operands{secrets};
    std::vector<const char *> names{"the secrets"};
    if (plaintexts) operands.push_back(plaintexts), names.push_back("the plaintexts");
    if (errors) operands.push_back(errors), names.push_back("the errors");
    for (size_t i = 0; i < P; ++i) operands.push_back(pubkeys[i]), names.push_back("a public key");
    const std::string overlap = row_outputs_overlap(outs, P, operands.data(), names.data(), operands.size());
    if (!overlap.empty()) return refuse(overlap);
    // last, so that a caller hears of a mistake in its operands first: what the Gaussian block sampler cannot serve - the
    // reference's keying, and a ring without a wave of lanes (two coefficients each) per polynomial chunk (sampling.hip)
    if (draws && ctx->env.rng_compat) return refuse("unsupported under MXX_HIP_RNG_COMPAT=reference");
    if (draws && ctx->N < 128) return refuse("unsupported: ring too small for a wave per polynomial chunk");
    return 0;
}

template <typename W, int VN>
int launch_main(GpuContext *ctx, const BggEncodeArgs &a, int ts, dim3 grid, dim3 block) {
#define MXX_BGG_ENCODE_TILE(TS) \
    if (ts == TS) MXX_LAUNCH((bgg_encode_kernel<W, VN, TS>), grid, block, 0, ctx->stream, a, ctx->d_limbs)
    MXX_BGG_ENCODE_TILE(1);
    MXX_BGG_ENCODE_TILE(2);
    MXX_BGG_ENCODE_TILE(4);
#undef MXX_BGG_ENCODE_TILE
    HIP_TRY(hipGetLastError());
    return 0;
}

// slots [s0, s0 + Sg) with their errors at `errors` (Sg x (P m) words, or null): the table in one staged copy, the kernel
int combine_group(const BggEncodeCall &call, GpuMatrix *const *outs, const GpuMatrix *secrets, const GpuMatrix *const *pubkeys,
                  const GpuMatrix *plaintexts, size_t s0, size_t Sg, const void *errors) {
    GpuContext *ctx = call.ctx;
    const size_t P = call.P, wpp = static_cast<size_t>(call.L) << ctx->logN, poly_bytes = wpp * ctx->word_bytes;
    static thread_local std::vector<uint64_t> staging;
    staging.resize(2 * P + static_cast<size_t>(call.L) * call.dpt);
    for (size_t i = 0; i < P; ++i) {
        staging[i] = reinterpret_cast<uint64_t>(static_cast<char *>(words_ptr(outs[i])) + s0 * call.m * poly_bytes);
        staging[P + i] = reinterpret_cast<uint64_t>(words_ptr(pubkeys[i]));
    }
    for (uint32_t l = 0; l < call.L; ++l) base_powers(ctx->moduli[l], call.base_bits, call.dpt, staging.data() + 2 * P + static_cast<size_t>(l) * call.dpt);
    CtxBlock block(ctx);
    if (upload_table(block, "BGG encoding table (host to device)", staging)) return 1;
    const size_t vn = ctx->N % (16 / ctx->word_bytes) == 0 ? 16 / ctx->word_bytes : 1;
    const int ts = slot_tile(Sg);
    BggEncodeArgs a;
    a.secrets = static_cast<const char *>(words_ptr(secrets)) + s0 * call.d * poly_bytes;
    a.plaintexts = plaintexts ? static_cast<const char *>(words_ptr(plaintexts)) + s0 * (P - 1) * poly_bytes : nullptr;
    a.errors = errors, a.table = static_cast<const uint64_t *>(block.ptr);
    a.m = call.m, a.k = call.k, a.entries = tile_entries(call, Sg);
    a.S = static_cast<uint32_t>(Sg), a.P = static_cast<uint32_t>(P), a.d = static_cast<uint32_t>(call.d);
    a.L = call.L, a.dpt = call.dpt, a.logN = ctx->logN, a.slot_tiles = static_cast<uint32_t>((Sg + ts - 1) / ts);
    const size_t vecs = static_cast<size_t>(ctx->N) / vn;
    size_t gy, gz;
    (void)fold_yz(a.entries, gy, gz);  // grid_plan.h; the count was held to 65535 x 65535 with the refusals
    const unsigned threads = static_cast<unsigned>(std::min<size_t>(256, (vecs + 63) / 64 * 64));
    const dim3 grid(static_cast<unsigned>(std::min<size_t>((vecs + threads - 1) / threads, 64)), static_cast<unsigned>(gy), static_cast<unsigned>(gz));
    // the errors read once and the outputs written once; A_i once per slot tile, T once per column (and once more in the
    // limb the gadget hits, with the plaintext)
    const double polys = static_cast<double>(Sg) * P * call.m;
    MXX_TRACE_BYTES(poly_bytes * (polys * (errors ? 2.0 : 1.0) + static_cast<double>(a.slot_tiles) * P * call.m * call.d + polys * call.d +
                                  polys * (P > 1 ? 2.0 : 1.0) / call.L));
    if (ctx->wide && vn > 1) return launch_main<uint64_t, 2>(ctx, a, ts, grid, dim3(threads));
    if (ctx->wide) return launch_main<uint64_t, 1>(ctx, a, ts, grid, dim3(threads));
    if (vn > 1) return launch_main<uint32_t, 4>(ctx, a, ts, grid, dim3(threads));
    return launch_main<uint32_t, 1>(ctx, a, ts, grid, dim3(threads));
}

// after the refusals: (*go) whether anything is left to launch; PACKED24 operands unpacked once.  The outputs' tags are set
// by tag_outputs once everything has been enqueued: a call that fails later (an allocation, a group's sampler) leaves them
int accept(const BggEncodeCall &call, GpuMatrix *const *outs, const GpuMatrix *secrets, const GpuMatrix *const *pubkeys, const GpuMatrix *plaintexts,
           const GpuMatrix *errors, bool *go) {
    *go = call.S != 0 && call.P != 0 && call.d != 0 && call.m != 0;
    if (!*go) return 0;
    if (ctx_activate(call.ctx)) return 1;
    words_ptr(secrets);
    for (size_t i = 0; i < call.P; ++i) words_ptr(pubkeys[i]), words_ptr(outs[i]);
    if (plaintexts) words_ptr(plaintexts);
    if (errors) words_ptr(errors);
    return 0;
}

int tag_outputs(const BggEncodeCall &call, GpuMatrix *const *outs, int rc) {
    if (rc == 0)
        for (size_t i = 0; i < call.P; ++i) outs[i]->format = GPU_POLY_FORMAT_EVAL;
    return rc;
}

}  // namespace

extern "C" int gpupoly_matrix_bgg_encode_slots(GpuMatrix *const *outs, size_t ninputs_P, const GpuMatrix *secrets, const GpuMatrix *const *pubkeys,
                                               const GpuMatrix *plaintexts, uint32_t base_bits, double sigma, const GpuRngSeed *seeds) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_bgg_encode_slots";
    const size_t P = ninputs_P;
    if (P == 0) return 0;
    BggEncodeCall call;
    if (check_call(who, outs, P, secrets, pubkeys, plaintexts, base_bits, true, sigma, seeds, nullptr, &call)) return 1;
    GpuContext *ctx = call.ctx;
    const bool draws = sigma > 0.0;
    const size_t poly_bytes = static_cast<size_t>(call.L) * ctx->N * ctx->word_bytes;
    // a slot's scratch: its error row 1 x P m and the int64 samples the Gaussian lane kernel stages for it
    const size_t e_bytes = call.P * call.m * poly_bytes;
    const size_t slot_bytes = std::max<size_t>(e_bytes + call.P * call.m * static_cast<size_t>(ctx->N) * sizeof(int64_t), 1);
    const size_t S = call.S, per_group = draws ? rows_per_group(S, slot_bytes, call.cap) : S;
    if (tile_entries(call, per_group) > kMaxVectors) return set_error(std::string(who) + ": too many output tiles in one group");
    if (draws && per_group * call.P * call.m >> 32) return set_error(std::string(who) + ": too many error polynomials in one group");
    // ---- accepted ----
    bool go;
    if (accept(call, outs, secrets, pubkeys, plaintexts, nullptr, &go)) return 1;
    if (!go) return tag_outputs(call, outs, 0);
    if (!draws) return tag_outputs(call, outs, combine_group(call, outs, secrets, pubkeys, plaintexts, 0, S, nullptr));
    CtxBlock errors(ctx);
    if (errors.alloc(per_group * e_bytes)) return 1;
    for (size_t s0 = 0; s0 < S; s0 += per_group) {
        const size_t Sg = std::min(per_group, S - s0);
        GpuMatrix e = scratch_matrix(ctx, call.level, Sg, call.P * call.m, errors.ptr);
        if (int rc = sample_blocks_impl(who, false, &e, GPU_MATRIX_DIST_GAUSS, seeds + s0, nullptr, Sg, GPUPOLY_BLOCKS_STACKED, nullptr, nullptr, &sigma))
            return rc;
        if (int rc = combine_group(call, outs, secrets, pubkeys, plaintexts, s0, Sg, errors.ptr)) return rc;
    }
    return tag_outputs(call, outs, 0);
    ABI_GUARD_END
}

// The same with the errors GIVEN (S x P m, EVAL) or absent (null) instead of sampled: the table copy and the kernel alone, one
// group.  A test instrument (tests/test_gpu_bgg_encode.py reaches the lazy accumulator's bound with errors no sampler gives),
// and what the host mirror calls with errors of the plain sampler where the block sampler is "unsupported".
extern "C" int gpupoly_matrix_bgg_encode_slots_combine(GpuMatrix *const *outs, size_t ninputs_P, const GpuMatrix *secrets,
                                                       const GpuMatrix *const *pubkeys, const GpuMatrix *plaintexts, uint32_t base_bits,
                                                       const GpuMatrix *errors) {
    ABI_GUARD_BEGIN
    static const char *const who = "gpupoly_matrix_bgg_encode_slots_combine";
    const size_t P = ninputs_P;
    if (P == 0) return 0;
    BggEncodeCall call;
    if (check_call(who, outs, P, secrets, pubkeys, plaintexts, base_bits, false, 0.0, nullptr, errors, &call)) return 1;
    if (tile_entries(call, call.S) > kMaxVectors) return set_error(std::string(who) + ": too many output tiles in one group");
    bool go;
    if (accept(call, outs, secrets, pubkeys, plaintexts, errors, &go)) return 1;
    if (!go) return tag_outputs(call, outs, 0);
    return tag_outputs(call, outs, combine_group(call, outs, secrets, pubkeys, plaintexts, 0, call.S, errors ? words_ptr(errors) : nullptr));
    ABI_GUARD_END
}
