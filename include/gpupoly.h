/*
 * gpupoly.h — C ABI of libgpupoly for AMD MI355X (gfx950).
 *
 * Drop-in boundary for the `gpu` feature of MachinaIO/mxx: every entry point
 * below replaces the function of the same name that mxx's Rust side binds in
 *   src/poly/dcrt/gpu.rs:69-240  (unsafe extern "C" block)
 * and that its CUDA tree declares in
 *   cuda/include/Runtime.cuh:20-44,108
 *   cuda/include/matrix/MatrixData.cuh:10-27
 *   cuda/include/matrix/MatrixArith.cuh:10-26
 *   cuda/include/matrix/MatrixNTT.cuh:9-10
 *   cuda/include/matrix/MatrixDecompose.cuh:26-37
 *   cuda/include/matrix/MatrixSampling.cuh:25-37
 *   cuda/include/matrix/MatrixTrapdoor.cuh:66-101
 *   cuda/include/matrix/MatrixSerde.cuh:10-58
 * (paths relative to the reference checkout).
 *
 * Conventions:
 *   - int-returning functions: 0 = ok, non-zero = error; the message is
 *     available from gpu_last_error() (thread-local, valid until the next
 *     error on that thread).  Nothing throws across this boundary.
 *   - *_create hands out an owning pointer; *_destroy is stream-ordered and
 *     may be called while device work on the object is still in flight.
 *   - handles may be used concurrently from several host threads.
 *   - compute entry points do not block the host; load/store *_batch return
 *     an event set (possibly NULL) the caller waits on and destroys;
 *     gpu_matrix_equal and the compact-bytes pair are synchronous.
 *   - device layout is private: words [poly][limb][N], poly = row*cols + col,
 *     uint32_t residues when every modulus is < 2^31, uint64_t otherwise.
 *   - EVAL format is OpenFHE's: slot k of limb i holds a(psi_i^(2*bitrev(k)+1))
 *     with psi_i the minimum primitive 2N-th root mod q_i (the reference CPU
 *     path's convention), so EVAL bytes are interchangeable with the CPU side.
 *   - operands that share memory.  "Overlap" always means byte ranges of device storage, never object identity: a
 *     row view (gpupoly_matrix_row_view) is another object over its parent's bytes and overlaps it.  "The same block"
 *     means the same object, or a view with the same start and the same byte length.
 *       1. Point-wise entries - gpu_matrix_add, gpu_matrix_sub, gpupoly_matrix_neg, gpu_matrix_mul_scalar,
 *          gpupoly_matrix_mul_scalar_intt (its lhs), gpupoly_matrix_scale_round, the ADD / SUB / NEG / MUL_SCALAR
 *          gates of gpupoly_batch and the addend of gpupoly_matrix_monomial_sum: an operand may be the same block as
 *          the output, and the result is the out-of-place one (for mul_scalar also the 1x1 out == lhs == scalar).
 *          Likewise the addend of gpupoly_matrix_mul_sum (gpupoly_matrix_mul_acc: `out` is its own addend); their
 *          lhss[t] / rhss[t] fall under 3.  Likewise the addend of gpupoly_matrix_mul_gadget and of
 *          gpupoly_matrix_gadget_mul; their lhs, scalar_1x1 and rhs fall under 3.  Likewise addends[j] against outs[j]
 *          in gpupoly_matrix_mul_decompose_gadget_scalar_many and gpupoly_matrix_mul_decompose_gadget_const_many.
 *       2. Any other overlap of their output with an operand is refused.
 *       3. Every other entry that reads matrices and writes one refuses any overlap between what it writes and what
 *          it reads, the same block included (gpu_matrix_gauss_samp_gq_arb_base before its source is transformed).
 *          gpupoly_matrix_add_rows / _ntt_add_rows are judged on the destination row block: an operand may be a view
 *          of other rows of `out`.  gpupoly_matrix_decompose_rows is judged like gpu_matrix_decompose_base: its `out`
 *          overlaps no byte of `src`, whichever rows the window reads.  In gpupoly_matrix_mul_decompose_gadget_scalar_many / _const_many no outs[j] overlaps
 *          any lhss[o], scalar_1x1, another output or another operand's addend.
 *       4. Several outputs: the blocks of gpupoly_matrix_split_columns are pairwise disjoint and disjoint from the
 *          source (the blocks of a concat may repeat, its output is disjoint from all of them); in
 *          gpupoly_matrix_mul_batch and gpupoly_batch no output overlaps another product's / gate's output or
 *          operand; gpupoly_matrix_all_gather_columns wants full[r] disjoint from local_blocks[r].
 *       5. gpu_matrix_copy_block / gpu_matrix_add_block give the result of reading the whole source block before the
 *          first write whenever `out` and `src` share storage (they stage it).  gpu_matrix_copy does nothing on the
 *          same block and refuses a partial overlap.
 *       6. Disjoint views of one parent are ordinary operands everywhere.
 *     A call refused under this rule launches nothing and leaves the residues and the format tag of every matrix
 *     passed to it as they were; its message names the entry point and contains "alias" or "overlap".
 *     INTEGRATION.md lists every entry point that takes two or more matrices with its case.
 */
#ifndef GPUPOLY_H
#define GPUPOLY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct GpuContext GpuContext;
typedef struct GpuMatrix GpuMatrix;
typedef struct GpuEventSet GpuEventSet;
typedef struct GpuP1CovarianceCache GpuP1CovarianceCache;
typedef struct GpuComm GpuComm; /* extension: communicator over the device contexts of ONE process */

/* src/poly/dcrt/gpu.rs:45-61, cuda/include/ChaCha.cuh:9-12 — passed BY VALUE */
typedef struct GpuRngSeed {
    uint64_t words[4];
} GpuRngSeed;

/* src/poly/dcrt/gpu.rs:242-247 */
#define GPU_POLY_FORMAT_COEFF 0
#define GPU_POLY_FORMAT_EVAL 1
#define GPU_MATRIX_DIST_UNIFORM 0
#define GPU_MATRIX_DIST_GAUSS 1
#define GPU_MATRIX_DIST_BIT 2
#define GPU_MATRIX_DIST_TERNARY 3
#define GPU_MATRIX_LAYOUT_WORDS 0    /* one 4- or 8-byte word per residue */
#define GPU_MATRIX_LAYOUT_PACKED24 1 /* 3 bytes per residue (moduli below 2^24): uniform samples, until first words use */

/* ---- runtime: cuda/include/Runtime.cuh:20-44,108 ------------------------- */
/* L = moduli_len - 1 (top level); gpu_ids[0] is the device the context lives on. */
int gpu_context_create(uint32_t logN, uint32_t L, uint32_t dnum, const uint64_t *moduli, size_t moduli_len,
                       const int *gpu_ids, size_t gpu_ids_len, GpuContext **out_ctx);
void gpu_context_destroy(GpuContext *ctx);
int gpu_context_get_N(const GpuContext *ctx, int *out_N);

int gpu_event_set_wait(GpuEventSet *events);
void gpu_event_set_destroy(GpuEventSet *events);

int gpu_device_count(int *out_count);
int gpu_device_mem_info(int device, size_t *out_free, size_t *out_total);
int gpu_device_synchronize(void);
int gpu_device_reset(void);

const char *gpu_last_error(void);
int gpu_set_last_error(const char *msg);

void *gpu_pinned_alloc(size_t bytes);
void gpu_pinned_free(void *ptr);

/* ---- storage: cuda/include/matrix/MatrixData.cuh:10-27 -------------------- */
/* contents undefined after create; a matrix at `level` uses limbs 0..=level */
int gpu_matrix_create(GpuContext *ctx, int level, size_t rows, size_t cols, int format, GpuMatrix **out);
void gpu_matrix_destroy(GpuMatrix *mat);
int gpu_matrix_copy(GpuMatrix *dst, const GpuMatrix *src);
/* gpu_matrix_copy_block / gpu_matrix_add_block: the window rule is offset <= extent and count <= extent - offset on each
 * of the four axes (an offset + count that wraps around size_t is out of bounds like any other); add_block takes at
 * most 65535 columns.  A successful call retags the whole of `out` with src's format, as the reference does; a refused
 * one - "source block out of bounds", "destination block out of bounds", "block too wide" - launches nothing and leaves
 * out's words and tag as they were.  The same holds for gpu_matrix_mul and gpupoly_matrix_fill_identity refused with
 * "matrix too large". */
int gpu_matrix_copy_block(GpuMatrix *out, const GpuMatrix *src, size_t dst_row, size_t dst_col, size_t src_row,
                          size_t src_col, size_t rows, size_t cols);

/* ---- arithmetic: cuda/include/matrix/MatrixArith.cuh:10-26 ---------------- */
int gpu_matrix_add(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs);
int gpu_matrix_sub(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs);
int gpu_matrix_add_block(GpuMatrix *out, const GpuMatrix *src, size_t dst_row, size_t dst_col, size_t src_row,
                         size_t src_col, size_t rows, size_t cols);
int gpu_matrix_mul(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs);          /* both EVAL */
int gpu_matrix_mul_scalar(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *scalar); /* scalar is 1x1, EVAL */
int gpu_matrix_equal(const GpuMatrix *lhs, const GpuMatrix *rhs, int *out_equal);

/* ---- NTT: cuda/include/matrix/MatrixNTT.cuh:9-10 (idempotent) -------------- */
int gpu_matrix_ntt_all(GpuMatrix *mat);
int gpu_matrix_intt_all(GpuMatrix *mat);

/* ---- gadget / decompose: cuda/include/matrix/MatrixDecompose.cuh:26-37 ---- */
int gpu_matrix_fill_gadget(GpuMatrix *out, uint32_t base_bits);
int gpu_matrix_fill_small_gadget(GpuMatrix *out, uint32_t base_bits);
int gpu_matrix_fill_small_decomposed_identity_chunk(GpuMatrix *out, const GpuMatrix *scalar_by_digit,
                                                    size_t chunk_idx);
int gpu_matrix_decompose_base(const GpuMatrix *src, uint32_t base_bits, GpuMatrix *out);
int gpu_matrix_decompose_base_small(const GpuMatrix *src, uint32_t base_bits, GpuMatrix *out);

/* ---- sampling: MatrixSampling.cuh:25-37, MatrixTrapdoor.cuh:66-101 --------- */
int gpu_matrix_sample_distribution(GpuMatrix *out, int dist_type, double sigma, GpuRngSeed seed);
int gpu_matrix_sample_distribution_columns(GpuMatrix *out, int dist_type, double sigma, GpuRngSeed seed,
                                           size_t full_ncol, size_t col_offset);
int gpu_matrix_gauss_samp_gq_arb_base(GpuMatrix *src, uint32_t base_bits, double c, double dgg_stddev,
                                      GpuRngSeed seed, GpuMatrix *out);
int gpu_matrix_sample_p1_full(const GpuMatrix *a_mat, const GpuMatrix *b_mat, const GpuMatrix *d_mat,
                              const GpuMatrix *tp2, double sigma, double s, double dgg_stddev, GpuRngSeed seed,
                              GpuMatrix *out);
int gpu_matrix_create_p1_covariance_cache(const GpuMatrix *a_mat, const GpuMatrix *b_mat, const GpuMatrix *d_mat,
                                          double sigma, double s, double dgg_stddev,
                                          GpuP1CovarianceCache **out_cache);
void gpu_matrix_destroy_p1_covariance_cache(GpuP1CovarianceCache *cache);
int gpu_matrix_sample_p1_full_cached(const GpuP1CovarianceCache *cache, const GpuMatrix *tp2, GpuRngSeed seed,
                                     GpuMatrix *out);

/* ---- serde: cuda/include/matrix/MatrixSerde.cuh:10-58 ---------------------- */
/* host layout [poly][limb][N] little-endian u64, poly stride = bytes_per_poly */
int gpu_matrix_load_rns_batch(GpuMatrix *mat, const uint8_t *bytes, size_t bytes_per_poly, int format,
                              GpuEventSet **out_events);
int gpu_matrix_store_rns_batch(const GpuMatrix *mat, uint8_t *bytes_out, size_t bytes_per_poly, int format,
                               GpuEventSet **out_events);
int gpu_matrix_store_const_coeff_batch(const GpuMatrix *mat, uint64_t *words_out, size_t words_per_poly,
                                       GpuEventSet **out_events);
/* compact wire format (coefficient-domain, CRT-reconstructed, centred, bit-packed at the matrix-wide width): the store
 * takes an EVAL matrix to the coefficient domain in place.  When payload_capacity is too small the call fails with
 * "payload buffer too small ..." AND reports the width / length it needs through the three out parameters (the
 * reference reports only the error), so a host need not reserve the worst case of bits(Q) per coefficient.       */
int gpu_matrix_store_compact_bytes(GpuMatrix *mat, uint8_t *payload_out, size_t payload_capacity,
                                   uint16_t *out_max_coeff_bits, uint16_t *out_bytes_per_coeff,
                                   size_t *out_payload_len);
int gpu_matrix_load_compact_bytes(GpuMatrix *mat, const uint8_t *payload, size_t payload_len,
                                  uint16_t max_coeff_bits);
int gpu_poly_store_compact_bytes(GpuMatrix *poly, uint8_t *payload_out, size_t payload_capacity,
                                 uint16_t *out_max_coeff_bits, uint16_t *out_bytes_per_coeff,
                                 size_t *out_payload_len);
int gpu_poly_load_compact_bytes(GpuMatrix *poly, const uint8_t *payload, size_t payload_len,
                                uint16_t max_coeff_bits);

/* ---- MI355X extensions (not in the reference ABI; prefixed gpupoly_) ------- */
/* S * G^-1(B) in one call (replaces the Rust-side loop src/matrix/gpu_dcrt_poly.rs:1414-1493, which re-reads S for
 * every column chunk): digits are generated inside the forward transform's load for all columns at once when
 * memory allows, then one product into `out`.  The EVAL-form digit matrix IS written once and read once (a full
 * fusion would need 8 x 16384 accumulators per workgroup).                          */
int gpupoly_matrix_mul_decompose(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs, uint32_t base_bits);
/* Several left operands against ONE G^-1(rhs), each with its addend (extension):
 *   outs[j] = lhss[j] * G^-1(rhs) + addends[j] o scalars[j]        for all j < n
 * - for every j the residues, bit for bit, of gpupoly_matrix_mul_decompose(tmp, lhss[j], rhs, base_bits),
 * gpu_matrix_mul_scalar(tmp2, addends[j], scalars[j]), gpu_matrix_add(outs[j], tmp, tmp2).  Replaces the repeated
 * decompositions of one matrix in the BGG multiplication gates: BggEncoding::mul (src/bgg/encoding.rs:125-145: vector and
 * public-key matrix against one other.pubkey.matrix, then + other.vector * plaintext), large_scalar_mul / matrix_mul
 * (:191-219), BggPolyEncoding::mul (src/bgg/poly_encoding.rs:327-357: one mul_decompose per slot, each followed by
 * + rhs_vector * lhs_plaintext, and one more for the keys at :341), src/io/diamond_io.rs:1924-1926 and
 * src/we/diamond_we.rs:456,538.  G^-1(rhs) is built ONCE per call with the fused digit transform - in as few column chunks
 * as the memory budget allows (the rule of gpupoly_matrix_mul_decompose; MXX_HIP_MUL_DECOMPOSE_MANY_BUDGET=<bytes>
 * overrides it for this entry) - and read by one grouped product per 64 operands and chunk, whose epilogue adds
 * addend o scalar and stores into each operand's own output: no stacking or splitting copies, no mul_scalar or add launch.
 *   rhs         r x c, COEFF or EVAL, left untouched (as with gpu_matrix_decompose_base); k = ceil(crt_bits/base_bits) * limbs
 *   lhss[j]     rows_j x (r*k), EVAL; rows_j may differ from operand to operand and may be 0
 *   outs[j]     rows_j x c, made by the caller, tagged EVAL on success
 *   addends     NULL, or addends[j] NULL: no addend; else rows_j x c, EVAL
 *   scalars     NULL, or scalars[j] NULL: the addend is added as it is; else 1 x 1, EVAL, multiplies every entry of
 *               addends[j] point-wise before the sum
 * One context and one level per call; n = 0 does nothing; r*k = 0 gives the addend term alone.  Enqueued on the context's
 * stream, the host does not block; temporaries come from the context's allocator and are released stream-ordered.
 * PACKED24 operands are unpacked first.  Every operand height goes through the grouped kernel in tiles of at most 8
 * stacked rows: it is built for few-row operands (encodings, key matrices of small d); operands of 24 rows and more are
 * better served by one gpupoly_matrix_mul_decompose each.
 * Refused, with nothing launched and every outs[j] (contents AND tag) untouched, all checked for every j before the first
 * launch: a null outs, lhss or rhs with n > 0, a null outs[j] or lhss[j]; a context or level mismatch or a shape mismatch
 * in any j; an lhss[j], addends[j] or scalars[j] not in EVAL form; a scalars[j] without an addends[j]; an output that
 * aliases any input or another output; base_bits of 0 or >= 63.                                                      */
int gpupoly_matrix_mul_decompose_many(GpuMatrix *const *outs, const GpuMatrix *const *lhss,
                                      const GpuMatrix *const *addends, const GpuMatrix *const *scalars, size_t n,
                                      const GpuMatrix *rhs, uint32_t base_bits);
/* Every left operand against ITS OWN G^-1 (extension):
 *   outs[j] = addends[j] (+|-) (lhss[j] * G^-1(rhss[j][:, col_start .. col_start + c))) o scalars[j]     j < n, c = outs[j]->cols
 * - for every j the residues, bit for bit, of gpu_matrix_copy_block of the window, gpupoly_matrix_mul_decompose,
 * gpu_matrix_mul_scalar, then gpu_matrix_add / gpu_matrix_sub / gpupoly_matrix_neg.  Replaces the per-request sequences of the
 * slot-transfer gate targets, build_gate_target_chunk_gpu and build_slot_reduce_gate_target_chunk_gpu
 * (src/slot_transfer/bgg_pubkey_gpu.rs:371-407,409-471), over the wave of requests that sample_gate_batch_gpu builds (:842):
 * the n windows are gathered into one r x (n c) matrix by one launch, ONE fused digit transform gives the (r k) x (n c) EVAL
 * digit matrix, and one grouped product per 64 operands reads operand j's panel [j c, (j + 1) c) of it, multiplies the
 * product by the scalar, adds it to or subtracts it from the addend and stores into the operand's own output.
 *   rhss[j]     r x m, COEFF or EVAL (they may differ), left untouched; all share r and m; only columns
 *               [col_start, col_start + c) are read; k = ceil(crt_bits/base_bits) * limbs
 *   lhss[j]     rows_j x (r*k), EVAL; rows_j may differ from operand to operand and may be 0
 *   outs[j]     rows_j x c, made by the caller, tagged EVAL on success; all share c
 *   addends     NULL, or addends[j] NULL: no addend; else rows_j x c, EVAL.  addends[j] may be outs[j]'s very block (the rule
 *               of gpupoly_matrix_mul_sum): every word is read and written by the same thread
 *   scalars     NULL, or scalars[j] NULL: the product as it is; else 1 x 1, EVAL.  It multiplies the PRODUCT, not the addend -
 *               the opposite of gpupoly_matrix_mul_decompose_many, whose scalar multiplies the addend
 *   negate      != 0 subtracts the product term; without an addend the output is then the negated product
 * One context and one level per call; n = 0 does nothing; r*k = 0 or c = 0 writes the addend term (or nothing) through the
 * same path.  Enqueued on the context's stream, the host does not block; temporaries come from the context's allocator and
 * are released stream-ordered.  PACKED24 operands are unpacked first.  When the digit matrix exceeds the budget rule of
 * gpupoly_matrix_mul_decompose_many (MXX_HIP_MUL_DECOMPOSE_PAIRS_BUDGET=<bytes> overrides it for this entry) the call is cut
 * into groups of operands.  The launch count does not depend on n up to 64 operands; every further 64 add one launch.
 * Refused, with nothing launched and every outs[j] (contents AND tag) untouched, all checked for every j before the first
 * launch: a null outs, lhss or rhss with n > 0, or a null entry in any of them; a context, level or shape mismatch in any j
 * (lhss[j]->cols != r*k, differing r, m or c, col_start + c > m); an lhss[j], addends[j] or scalars[j] not in EVAL form; an
 * output that aliases any input or another output, row views included - an addend that is its output's very block is the one
 * exception; base_bits of 0 or >= 63.                                                                                */
int gpupoly_matrix_mul_decompose_pairs(GpuMatrix *const *outs, const GpuMatrix *const *addends,
                                       const GpuMatrix *const *lhss, const GpuMatrix *const *rhss,
                                       const GpuMatrix *const *scalars, size_t n,
                                       size_t col_start, uint32_t base_bits, int negate);
/* outs[i] = lhss[i] * rhss[i], i < count: independent products of one context and level (all EVAL) in one call.  Small
 * products - a level of circuit gates on a small ring, where every product is a launch-latency-bound kernel - go out
 * up to 64 per launch; large ones run one by one through the tuned kernels.  No output may be another product's
 * operand.  (the reference issues one call per gate, src/circuit/poly_circuit/eval.rs:269.)        */
int gpupoly_matrix_mul_batch(GpuMatrix *const *outs, const GpuMatrix *const *lhss, const GpuMatrix *const *rhss, size_t count);
/* A level of independent circuit gates in one call (the reference issues one ABI call per gate,
 * src/circuit/poly_circuit/eval.rs:269-345): products go out up to 64 per launch (gpupoly_matrix_mul_batch), the
 * point-wise gates - add, sub, negate, product by a 1x1 ring element (Small / LargeScalarMul) - up to 64 per launch,
 * decompositions through their tuned paths.  One context; no output may be another gate's operand or output; formats
 * and shapes as for the single-gate entry points named below.  The matrices of a gate share one level (the MUL gates of
 * a call one level among themselves): a gate of mixed levels is refused with "level mismatch" before anything is
 * launched, whatever the other gates of the call are.                                                              */
#define GPUPOLY_OP_MUL 0           /* gpu_matrix_mul(out, lhs, rhs) */
#define GPUPOLY_OP_ADD 1           /* gpu_matrix_add(out, lhs, rhs); out may be lhs */
#define GPUPOLY_OP_SUB 2           /* gpu_matrix_sub */
#define GPUPOLY_OP_MUL_SCALAR 3    /* gpu_matrix_mul_scalar(out, lhs, rhs = 1x1) */
#define GPUPOLY_OP_NEG 4           /* gpupoly_matrix_neg(out, lhs); rhs ignored */
#define GPUPOLY_OP_DECOMPOSE 5     /* gpu_matrix_decompose_base(lhs, base_bits, out); rhs ignored */
#define GPUPOLY_OP_MUL_DECOMPOSE 6 /* gpupoly_matrix_mul_decompose(out, lhs, rhs, base_bits) */
typedef struct GpuBatchOp {
    int kind;
    GpuMatrix *out;
    const GpuMatrix *lhs;
    const GpuMatrix *rhs;
} GpuBatchOp;
int gpupoly_batch(const GpuBatchOp *ops, size_t count, uint32_t base_bits);
/* lhs * small-G^-1(rhs) (digits of limb 0 only): replaces the column-chunk loop of mul_decompose_small
 * (src/matrix/gpu_dcrt_poly.rs:1495-1574).                                                                */
int gpupoly_matrix_mul_decompose_small(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs, uint32_t base_bits);
/* lhs * (I_identity_size (x) rhs): one product per identity block, written in place, no slice / concat copies for
 * row-vector operands (replaces src/matrix/gpu_dcrt_poly.rs:1374-1390).                                     */
int gpupoly_matrix_mul_tensor_identity(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs, size_t identity_size);
/* lhs * (I_identity_size (x) G^-1(rhs)): G^-1(rhs) is built ONCE and reused by every identity block; the reference
 * decomposes every column again for every block (src/matrix/gpu_dcrt_poly.rs:1392-1412).                    */
int gpupoly_matrix_mul_tensor_identity_decompose(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs,
                                                 size_t identity_size, uint32_t base_bits);
/* out <- INTT(lhs o scalar_1x1): the point-wise product rides in the inverse transform's load (one HBM round
 * trip instead of two; replaces gpu_matrix_mul_scalar + gpu_matrix_intt_all).  out may be lhs.           */
int gpupoly_matrix_mul_scalar_intt(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *scalar_1x1);
/* out = src^T in one launch (the reference's wrapper issues rows*cols single-polynomial copy_block calls,
 * src/matrix/gpu_dcrt_poly.rs:1190-1199).                                                                */
int gpupoly_matrix_transpose(GpuMatrix *out, const GpuMatrix *src);
/* Constants written on the device instead of uploaded as full-size host byte vectors
 * (src/matrix/gpu_dcrt_poly.rs:343-365 `new_zero_with_state`, :1158-1188 `identity`).  fill_zero keeps the format
 * tag; fill_identity puts scalar_1x1 (EVAL; NULL = the constant 1) on the diagonal and tags the result EVAL.  */
/* out = lhs (x) rhs (Kronecker product, all EVAL) in one launch; the reference's wrapper runs an entry slice, a
 * mul_scalar and a copy_block per entry of lhs (src/matrix/gpu_dcrt_poly.rs:1225-1252).                     */
int gpupoly_matrix_tensor(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs);
/* out[dst_row .. dst_row + lhs.rows) = lhs + rhs: the sum lands in a row block of a taller matrix (contiguous in
 * the row-major layout) instead of a copy_block followed by an add_block; used by the preimage's final assembly
 * (src/sampler/trapdoor/gpu.rs:340-369).  The whole destination takes the operands' format tag.            */
int gpupoly_matrix_add_rows(GpuMatrix *out, size_t dst_row, const GpuMatrix *lhs, const GpuMatrix *rhs);
/* out[dst_row .. dst_row + coeff.rows) = NTT(coeff) + addend: `coeff` is a COEFF matrix, `addend` an EVAL matrix of the
 * same shape; transform, sum and placement are one pass at n = 2^14 with 32-bit words.  Elsewhere, consume_coeff != 0
 * (the caller gives `coeff` up: contents and tag unspecified afterwards) lets the library transform it in place and add
 * in a second pass; with consume_coeff == 0 `coeff` is left untouched at the price of a copy.  The preimage's bottom
 * block p2 + z (src/sampler/trapdoor/gpu.rs:340-369).  The whole destination is tagged EVAL.               */
int gpupoly_matrix_ntt_add_rows(GpuMatrix *out, size_t dst_row, GpuMatrix *coeff, const GpuMatrix *addend,
                                int consume_coeff);
/* A matrix object over rows [row, row + rows) of m (contiguous in the row-major layout) that SHARES m's storage - an
 * operand without the copy a slice makes.  Destroy it with gpu_matrix_destroy (the storage stays m's) before m.  */
int gpupoly_matrix_row_view(GpuMatrix *m, size_t row, size_t rows, GpuMatrix **out_view);
/* The same for the whole of m under another shape (extension): a rows x cols matrix object over ALL of
 * m's storage, rows * cols == m->rows * m->cols, entry (i, j) of the view = polynomial i * cols + j of m's row-major
 * order.  Its rules are gpupoly_matrix_row_view's: it shares words (a PACKED24 m is unpacked first and stays in words
 * while a view lives), carries its own format tag initialised from m's, and is destroyed with gpu_matrix_destroy before
 * m.  The overlap rule sees it through its byte range: it is the same block as m, and overlaps every view of m.
 * Refused, with nothing launched: a null argument; a polynomial count that differs.                               */
int gpupoly_matrix_reshape_view(GpuMatrix *m, size_t rows, size_t cols, GpuMatrix **out_view);
/* out = -src in one pass (the reference's wrapper: upload zeros, clone, subtract - gpu_dcrt_poly.rs:1890-1897). */
int gpupoly_matrix_neg(GpuMatrix *out, const GpuMatrix *src);
int gpupoly_matrix_fill_zero(GpuMatrix *out);
int gpupoly_matrix_fill_identity(GpuMatrix *out, const GpuMatrix *scalar_1x1);
/* G^-1 of a freshly sampled rows x cols matrix: out is (rows*k) x cols, k = digits per entry (small != 0: the digits
 * of limb 0 only).  Same samples as gpu_matrix_sample_distribution, same digits as gpu_matrix_decompose_base(_small);
 * the sample's NTT and the decomposition's copy + INTT are skipped (replaces the pairs in
 * src/sampler/gpu.rs:91-115, `sample_hash_decomposed` / `sample_hash_small_decomposed`).                   */
int gpupoly_matrix_sample_decomposed(GpuMatrix *out, int dist_type, double sigma, GpuRngSeed seed, uint32_t base_bits,
                                     int small);
/* A row window of a decomposition: out (R x c, c == src->cols) = rows [row_start, row_start + R) of D = G^-1(src), the
 * (src->rows * k) x c matrix gpu_matrix_decompose_base (small != 0: _small) writes - L = limbs of out's level, dpt =
 * ceil(crt_bits / base_bits), k = small ? dpt : dpt * L, row j*k + t*dpt + e of D = digit e of tower t of src[j, .]
 * (small: row j*dpt + e, tower 0).  The window rule: row_start + R <= src->rows * k, and the window may start and end
 * anywhere - inside a tower's digit block, across towers, across source rows.  Bit for bit the result of
 * gpu_matrix_decompose_base(_small) followed by gpu_matrix_copy_block of those rows, `out` keeping the format it was
 * created with (EVAL or COEFF), but the digit transforms - the cost of a decomposition - run for the R rows kept only:
 * the reference builds all r*k digit rows and slices (decompose_chunk / small_decompose_chunk of its matrix type; the
 * rhs_full.slice(inner_start, ..) of src/lookup/ggh15/poly_encoding_gpu.rs:515,566).  src is COEFF or EVAL and is left
 * untouched (a PACKED24 src is unpacked first); of an EVAL src only the source rows the window touches are inverse-
 * transformed into scratch, which comes from the context's allocator, is released stream-ordered and is sized by the
 * window.  Enqueued on the context's stream; the host does not block.  R = 0 or c = 0 succeed with nothing launched
 * (`out` tagged EVAL, as gpu_matrix_decompose_base tags an empty result).
 * Overlap: rule 3 - `out` must not overlap `src`, row views included (the message contains "overlap").
 * Refused, with nothing launched and `out` (contents AND tag) untouched, everything checked before the first launch,
 * the message naming this entry: a null matrix; base_bits of 0 or >= 63; a context, level or column mismatch; a window
 * past src->rows * k; `out` overlapping `src`.                                                                        */
int gpupoly_matrix_decompose_rows(const GpuMatrix *src, uint32_t base_bits, int small, size_t row_start, GpuMatrix *out);
/* The same window of the decomposition of a SAMPLED matrix: out (R x c) = rows [row_start, row_start + R) of G^-1 of
 * columns [col_offset, col_offset + c) of the src_rows x full_ncol matrix gpu_matrix_sample_distribution(seed) fills.
 * The window rule: col_offset + c <= full_ncol and row_start + R <= src_rows * k (k as above, from out's level).  Bit
 * for bit gpu_matrix_sample_distribution_columns + gpu_matrix_decompose_base(_small) + gpu_matrix_copy_block, for every
 * dist_type, under the default keying and under MXX_HIP_RNG_COMPAT=reference.  Only the source rows the window touches
 * are sampled and, for the uniform distribution (whose limbs are keyed separately), only the towers it touches when
 * the window lies inside one source row; the samples stay coefficients, no source transform runs in either direction.
 * This is what every production caller asks for: sample_hash_decomposed_columns / sample_hash_small_decomposed_columns
 * take a column chunk of a conceptual d x m_g matrix (src/lookup/ggh15/pubkey_gpu.rs:398-407,495-504,
 * src/lookup/ggh15/poly_encoding_gpu.rs:453-462,520-543; also ggh15/encoding.rs, ggh15/pubkey.rs, lwe/utils.rs,
 * src/slot_transfer/bgg_poly_encoding_gpu.rs) and poly_encoding_gpu.rs:515,566 keep rows [inner_start, inner_start +
 * inner_len) of it.  Stream, scratch and empty-window behaviour as gpupoly_matrix_decompose_rows.
 * Overlap: the only matrix is `out`; nothing can overlap.
 * Refused, with nothing launched and `out` (contents AND tag) untouched, everything checked before the first launch,
 * the message naming this entry: a null `out`; base_bits of 0 or >= 63; an invalid dist_type; a Gaussian sigma that is
 * not positive; a window past src_rows * k or past full_ncol; src_rows * full_ncol beyond the samplers' 48-bit stream
 * ids.                                                                                                               */
int gpupoly_matrix_sample_decomposed_window(GpuMatrix *out, int dist_type, double sigma, GpuRngSeed seed,
                                            uint32_t base_bits, int small, size_t src_rows, size_t full_ncol,
                                            size_t col_offset, size_t row_start);
/* hipEvent timing on the context's compute stream (bench.py's roofline leg). */
int gpupoly_timer_start(GpuContext *ctx);
int gpupoly_timer_stop(GpuContext *ctx, float *out_ms);
/* Non-blocking event marks on the compute stream (slot < 65536) and the elapsed
 * time between two marks once both have completed (blocks on the later one).    */
int gpupoly_timer_mark(GpuContext *ctx, uint32_t slot);
int gpupoly_timer_elapsed(GpuContext *ctx, uint32_t slot_begin, uint32_t slot_end, float *out_ms);
/* raw device pointer / byte size of a matrix (zero-copy interop, e.g. RCCL).  Always the words layout: a
 * GPU_MATRIX_LAYOUT_PACKED24 matrix is unpacked first (once, on its context's stream) and stays in words.  */
int gpupoly_matrix_device_ptr(const GpuMatrix *mat, void **out_ptr, size_t *out_bytes);
/* storage layout of a matrix now: GPU_MATRIX_LAYOUT_WORDS, or GPU_MATRIX_LAYOUT_PACKED24 - a uniform sample of a
 * 32-bit context whose moduli are all below 2^24 (MXX_HIP_PACK24=0 turns it off).  Any operation without a packed
 * path unpacks the matrix to words first; only the register-tile product reads the packed bytes.  */
int gpupoly_matrix_layout(const GpuMatrix *mat, int *out);
/* Replica of `src` in another context (same ring; any device): one device-to-device / peer copy over
 * xGMI, ordered on both contexts' streams - replaces the reference's host round trip
 * to_cpu_staging_bytes -> from_cpu_staging_bytes (src/lookup/ggh15/pubkey_gpu.rs:153-196).     */
int gpupoly_matrix_copy_to_context(GpuContext *dst_ctx, const GpuMatrix *src, GpuMatrix **out);
int gpupoly_context_device(const GpuContext *ctx, int *out_device);
int gpupoly_context_word_bytes(const GpuContext *ctx, int *out_bytes);
/* name of the product kernel the dispatcher launched for the last gpu_matrix_mul on this context (bench.py labels its
 * roofline with what actually ran); "" before the first product                                                  */
const char *gpupoly_context_last_kernel(const GpuContext *ctx);
/* the context's compute stream (hipStream_t): lets the host order collectives against engine work on the device */
int gpupoly_context_stream(const GpuContext *ctx, void **out_stream);
/* ---- multi-GPU exchange, one process / N device contexts ----------------------------------------
 * The reference runs ONE process with a context per device (`params_for_device`, src/poly/dcrt/gpu.rs:531-557) and
 * rayon over them (`preimage_batched_sharded`, src/sampler/trapdoor/gpu.rs:371-397); whatever has to exist on another
 * device travels through host bytes.  A communicator binds such contexts (the same ring on every one).  Backend
 * "rccl": ncclCommInitAll over the contexts' devices (librccl is loaded when the first communicator is created),
 * collectives enqueued on each context's own stream, xGMI between the devices.  Backend "peer": device-to-device
 * pulls ordered by events - chosen when contexts share a device (RCCL refuses that) or with MXX_HIP_COMM=peer.     */
int gpupoly_comm_create(GpuContext *const *ctxs, size_t n, GpuComm **out_comm);
void gpupoly_comm_destroy(GpuComm *comm);
int gpupoly_comm_size(const GpuComm *comm, int *out_size);
const char *gpupoly_comm_backend(const GpuComm *comm); /* "rccl" or "peer" */
/* All-gather of the column blocks of a column-sharded matrix: local_blocks[r] (rows x c_r, in context r, any format,
 * the same one everywhere) lands in columns [c_0 + .. + c_(r-1), +c_r) of full[s] (rows x sum c_r, in context s) for
 * every s; full[s] takes the blocks' format tag.  Shards may be uneven or empty.  Enqueued on the contexts' streams
 * behind whatever produced the blocks; the host does not block; a block may be overwritten or destroyed right after
 * the call.  One row and equal shards gather straight into full[s]; other shapes go through a padded staging block
 * of the context's allocator.  One collective at a time per communicator (calls serialise on its mutex); other host
 * threads may keep enqueueing work on the contexts' streams meanwhile, as long as nothing enqueued after the call
 * writes a block that was passed to it before the call returns.  The outputs' format tags change only on success. */
int gpupoly_matrix_all_gather_columns(GpuComm *comm, const GpuMatrix *const *local_blocks, GpuMatrix *const *full);
/* ---- several independent requests in one launch (replaces the rayon fan-out of small requests,
 * src/sampler/trapdoor/gpu.rs:371-397, whose callers - src/lookup/ggh15/pubkey_gpu.rs:615-971 - hand it dozens of
 * few-column targets against one trapdoor).  A matrix is read as the column-wise concatenation of `nseg` segments
 * (1..64), segment j = the next seg_cols[j] columns, with its own seed seeds[j]; the columns of segment j come out
 * bit for bit as the plain entry point writes them for a matrix made of those columns alone under seeds[j] (every
 * element's stream is keyed by its position inside its segment).  Gaussian distribution / trapdoor dimension <= 4 /
 * at most four digits per tower / n a multiple of 64 (128 for _sample_distribution_segments); anything else returns
 * an error whose text contains "unsupported" and the caller issues the requests one by one.                      */
int gpupoly_matrix_sample_distribution_segments(GpuMatrix *out, int dist_type, double sigma, const GpuRngSeed *seeds,
                                                const size_t *seg_cols, size_t nseg);
int gpupoly_matrix_sample_p1_full_cached_segments(const GpuP1CovarianceCache *cache, const GpuMatrix *tp2,
                                                  const GpuRngSeed *seeds, const size_t *seg_cols, size_t nseg,
                                                  GpuMatrix *out);
int gpupoly_matrix_gauss_samp_gq_arb_base_segments(GpuMatrix *src, uint32_t base_bits, double c, double dgg_stddev,
                                                   const GpuRngSeed *seeds, const size_t *seg_cols, size_t nseg,
                                                   GpuMatrix *out);
/* Uniform / bit / ternary samples of `nblk` independently seeded blocks in one call (extension): the
 * tagged sample_hash loops of src/commit/wee25.rs:687-703,858-883, src/lookup/ggh15/pubkey_gpu.rs:924,1296 and
 * src/lookup/lwe/pubkey_gpu.rs:559,616, which draw one small matrix per index.  nblk is 1..2^20, not bounded by the 64
 * segments of the Gaussian entries: the sub-keys (nblk x limbs for the uniform distribution, nblk otherwise) and the
 * segment starts live in a table from the context's allocator, released stream-ordered, and the number of launches
 * (key derivation, sampling, transform or pack) does not depend on nblk.  `seeds` (nblk of them) are read before the
 * call returns.  Every sample is the plain entry's: the default keying of gpu_matrix_sample_distribution, with the
 * polynomial's index INSIDE its block as the stream id.
 *   GPUPOLY_BLOCKS_STACKED (seg_cols == NULL): out is nblk x P; row t holds, bit for bit, the P polynomials
 *       gpu_matrix_sample_distribution writes into any r x c matrix with r * c == P under seeds[t], in row-major
 *       order (the local index is the column).  sum_t W_t o a_t is then the one-row product [a_0 .. a_(nblk-1)] * out.
 *   GPUPOLY_BLOCKS_COLUMNS: out = [S_0 | S_1 | ...], S_j = out->rows x seg_cols[j] = what the plain entry writes for a
 *       matrix of that shape under seeds[j] (the local index is row * seg_cols[j] + local column): the semantics of
 *       gpupoly_matrix_sample_distribution_segments.
 * `out` ends as the plain entry leaves it: tagged EVAL, at its own level, GPU_MATRIX_LAYOUT_PACKED24 where a uniform
 * sample of the plain entry would be.  Enqueued on the context's stream; the host does not block.  An `out` without
 * polynomials succeeds with nothing launched and is tagged EVAL.
 * Overlap: the only matrix is `out`; nothing can overlap.
 * Refused, with nothing launched and `out` (contents AND tag) untouched, the message naming this entry: a null `out` or
 * `seeds`; nblk == 0 or above 2^20; an unknown layout; STACKED with seg_cols != NULL or out->rows != nblk; COLUMNS with
 * a null seg_cols, a zero width or widths that do not sum to out->cols; an invalid dist_type; a block of 2^48
 * polynomials or more (the 48-bit stream ids).  Refused likewise with an error containing "unsupported": the Gaussian
 * distribution (gpupoly_matrix_sample_gauss_blocks, below, is its entry); a context created under
 * MXX_HIP_RNG_COMPAT=reference (issue the requests one by one).
 * gpupoly_matrix_sample_hash_blocks is this entry with the seeds hashed from (key, tags) on the device.          */
#define GPUPOLY_BLOCKS_STACKED 0
#define GPUPOLY_BLOCKS_COLUMNS 1
int gpupoly_matrix_sample_distribution_blocks(GpuMatrix *out, int dist_type, const GpuRngSeed *seeds, size_t nblk,
                                              int layout, const size_t *seg_cols);
/* ---- tags to seeds on the device (extension).  The tagged loops above begin on the host with one hash
 * per tag: hash_seed_for_matrix (src/sampler/gpu.rs:118-136) is H("GpuDCRTPolyHashSampler/v2" || key || tag || ctr_le32),
 * H = Keccak-256 (the original 0x01 padding) in every instantiation of the reference, its 32-byte digest read as four
 * little-endian words (GpuRngSeed::from_bytes); the counter loop runs once, with counter 0.  A GpuHashTags names the hash,
 * the 32-byte key and the tags t = 0 .. count - 1 (the count is the entry's argument) in one of three forms:
 *   GPUPOLY_TAGS_TABLE            tag t = tags[tag_offsets[t] .. tag_offsets[t + 1]): any bytes, any lengths, empty tags
 *                                 included; tag_offsets has count + 1 entries, starts at 0 and does not decrease.  `tags`
 *                                 may be NULL when every tag is empty.  Bytes and offsets go up in one staged copy and are
 *                                 not read after the call returns.
 *   GPUPOLY_TAGS_INDEXED_LE64     tag t = tags[0 .. prefix_len) || (first_index + t) as 8 little-endian bytes: the
 *                                 b"wee25_w_block_" || idx.to_le_bytes() of src/commit/wee25.rs:687-703,858-883.
 *   GPUPOLY_TAGS_INDEXED_DECIMAL  tag t = the prefix || first_index + t in ASCII decimal without leading zeros (1 to 20
 *                                 digits): the format!("ggh15_lut_v_idx_{}_{}", lut_id, idx) of
 *                                 src/lookup/ggh15/pubkey_gpu.rs:398-401,924,1296 and src/lookup/lwe/pubkey_gpu.rs:559,616
 *                                 with "ggh15_lut_v_idx_<lut_id>_" as the prefix.
 * In the indexed forms prefix_len is at most 64, tag_offsets is NULL, first_index + count - 1 must not wrap, the prefix
 * travels by value with the launch and the tags are generated on the device: O(1) host work, nothing uploaded.       */
#define GPUPOLY_HASH_KECCAK256 0 /* padding byte 0x01: keccak_asm::Keccak256 */
#define GPUPOLY_HASH_SHA3_256 1  /* padding byte 0x06: FIPS 202 */
#define GPUPOLY_TAGS_TABLE 0
#define GPUPOLY_TAGS_INDEXED_LE64 1
#define GPUPOLY_TAGS_INDEXED_DECIMAL 2
typedef struct GpuHashTags {
    int hash; /* GPUPOLY_HASH_* */
    int form; /* GPUPOLY_TAGS_* */
    uint8_t key[32];
    const uint8_t *tags;       /* TABLE: the packed tag bytes; INDEXED: the prefix */
    const size_t *tag_offsets; /* TABLE only */
    size_t prefix_len;         /* INDEXED only */
    uint64_t first_index;      /* INDEXED only */
} GpuHashTags;
/* seeds_out[t] = hash_seed_for_matrix(key, tag_t) for t < ntags (1..2^20), one device lane per tag; blocks until the
 * seeds are in host memory.  The entry behind the mirror's single-tag calls, and the instrument the tests read the device
 * hash with.  No state of the context is involved: any context of a device gives the same seeds.
 * Refused, the message naming this entry and nothing launched: a null ctx, tags or seeds_out; ntags == 0 or above 2^20;
 * an unknown hash or form; TABLE with a null tag_offsets, tag_offsets[0] != 0, decreasing offsets, or null tags unless all
 * tags are empty; INDEXED with prefix_len > 64, a null prefix of non-zero length, a non-null tag_offsets or a wrapping
 * index range.                                                                                                     */
int gpupoly_hash_seeds(GpuContext *ctx, const GpuHashTags *tags, size_t ntags, GpuRngSeed *seeds_out);
/* gpupoly_matrix_sample_distribution_blocks with seeds[t] = hash_seed_for_matrix(key, tag_t), t < nblk, derived on the
 * device by one launch in front of the same key-derivation, sampling and transform / pack launches: the seeds never exist
 * on the host.  `out` ends bit for bit as that entry leaves it for the host-derived seeds (same tag, same level, same
 * PACKED24 rule); layout and seg_cols mean what they mean there.  In the TABLE form tag bytes, offsets and the columns
 * layout's starts go up in one staged copy; in the indexed forms only the columns layout's starts go up, the stacked layout
 * copies nothing.  Enqueued on the context's stream; the host does not block.
 * Overlap: the only matrix is `out`; nothing can overlap.
 * Refused, with nothing launched and `out` (contents AND tag) untouched, the message naming this entry: everything
 * gpupoly_matrix_sample_distribution_blocks refuses (the Gaussian distribution and MXX_HIP_RNG_COMPAT=reference with
 * "unsupported") and everything gpupoly_hash_seeds refuses of `tags`.                                                 */
int gpupoly_matrix_sample_hash_blocks(GpuMatrix *out, int dist_type, const GpuHashTags *tags, size_t nblk, int layout,
                                      const size_t *seg_cols);
/* ---- Gaussian seeded blocks (extension).  Replaces the per-request `sample_error_matrix`
 * (src/lookup/ggh15/pubkey.rs:227-239; its calls at pubkey_gpu.rs:428,457,476,507,535: one freshly seeded Gaussian matrix
 * per gate, stage and column chunk) and the GaussDist calls of `US::sample_uniform` in the gate stages and in
 * src/bgg/sampler_gpu.rs:125-135, one derive / sample / scatter / transform sequence each.
 * out = the blocks of gpupoly_matrix_sample_distribution_blocks (same layouts, same nblk 1..2^20, same seg_cols rules),
 * block t bit for bit what gpu_matrix_sample_distribution(GAUSS, sigma, seeds[t]) writes for that block alone; ends EVAL,
 * at its own level, in plain words (a Gaussian sample is never stored packed).  Four launches whatever nblk is: key
 * derivation, the lane sampler, the scatter of its integers into residues, the forward transform.  Enqueued on the
 * context's stream; the host does not block.  An `out` without polynomials succeeds with nothing launched, tagged EVAL.
 * Overlap: the only matrix is `out`; nothing can overlap.
 * Refused, with nothing launched and `out` (contents AND tag) untouched, the message naming this entry: everything
 * gpupoly_matrix_sample_distribution_blocks refuses for its layouts (MXX_HIP_RNG_COMPAT=reference with "unsupported");
 * sigma not > 0 ("sigma must be positive"); a ring of n < 128, whose polynomials hold less than a wave's 64 pairs
 * ("unsupported": issue the requests one by one); more than 2^32 polynomials.                                      */
int gpupoly_matrix_sample_gauss_blocks(GpuMatrix *out, double sigma, const GpuRngSeed *seeds, size_t nblk, int layout,
                                       const size_t *seg_cols);
/* the same with the seeds hashed from (key, tags) on the device, as gpupoly_matrix_sample_hash_blocks: one launch in
 * front, five in all; the Gaussian matrices of the tagged loops (`sample_hash` with GaussDist) and the hashed error
 * blocks of the gate stages.  Refused likewise, plus everything gpupoly_hash_seeds refuses of `tags`.               */
int gpupoly_matrix_sample_hash_gauss_blocks(GpuMatrix *out, double sigma, const GpuHashTags *tags, size_t nblk, int layout,
                                            const size_t *seg_cols);
/* out = [blocks[0] | blocks[1] | ...] / blocks[j] = the next blocks[j]->cols columns of src, in one launch per 64
 * blocks (the wrapper's concat_columns / slice_columns are a gpu_matrix_copy_block launch per block,
 * src/matrix/gpu_dcrt_poly.rs:1216-1260).  Same rows, level and context everywhere; the written side takes the read
 * side's format tag.                                                                                              */
int gpupoly_matrix_concat_columns(GpuMatrix *out, const GpuMatrix *const *blocks, size_t n);
int gpupoly_matrix_split_columns(const GpuMatrix *src, GpuMatrix *const *blocks, size_t n);
/* Several preimage requests against ONE trapdoor in one call: x_j with A x_j = targets[j] for j < n - for every request
 * the SAME matrix, bit for bit, that the one-request preimage (src/sampler/trapdoor/gpu.rs:228-369) produces for
 * targets[j] alone under the seeds seeds[3j] (p2), seeds[3j+1] (p1), seeds[3j+2] (z).  Replaces the per-request loop
 * of preimage_batched_sharded (gpu.rs:371-397) for one key group.
 *   re            [R; E] of the trapdoor, 2d x dk, EVAL (dk = d * digits per tower * limbs)
 *   cache         the trapdoor's p1 covariance cache; it carries the widths c = cache sigma, s and dgg_stddev, and
 *                 the large width is sqrt(s*s - c*c)
 *   public_matrix A = [left | right], d x (2d + dk), EVAL
 *   targets[j]    d x cols_j, EVAL;  outs[j]: (2d + dk) x cols_j, made by the caller, tagged EVAL on success
 * The requests go out in groups of up to 64 (p2 capped at 1 GiB per group), each group one sequence of launches:
 * p1 and p2 sampled into one stacked matrix P = [p1; p2] (padded per request to a multiple of d columns), A P as one
 * product, u - A P by one gather over the targets, the G-sampler, [R;E] z, and one scatter of
 * [P_top + [R;E] z ; P_bottom + z] into the outputs.  Temporaries come from the context's allocator and are released
 * stream-ordered; the host does not block.  Zero-column requests give zero-column outputs; n = 0 does nothing.
 * A refused call launches nothing and writes no output, not even a format tag: context or level mismatch, wrong
 * shapes, a target not in EVAL form, an output that aliases an input or another output.  Shapes the segmented
 * samplers do not cover (n not a multiple of 128, d > 4, more than four digits per tower, MXX_HIP_RNG_COMPAT=reference,
 * MXX_HIP_P1=simple) are refused with an error whose text contains "unsupported": issue those requests one by one. */
int gpupoly_trapdoor_preimage_many(const GpuMatrix *re, const GpuP1CovarianceCache *cache, const GpuMatrix *public_matrix,
                                   uint32_t base_bits, const GpuMatrix *const *targets, size_t n, const GpuRngSeed *seeds,
                                   GpuMatrix *const *outs);
/* The same for requests that do NOT all share a trapdoor: request j belongs to key key_of[j] < nkeys and outs[j] is, bit for
 * bit, what gpupoly_trapdoor_preimage_many writes for targets[j] alone with (res[k], caches[k], public_matrices[k]),
 * k = key_of[j], under the seeds seeds[3j], seeds[3j+1], seeds[3j+2] - whatever the spread of the requests over the keys,
 * their order, or what else is in the call.  Replaces the body of preimage_batched_sharded (gpu.rs:371-397) for one
 * context: its requests each carry their own (trapdoor, public matrix, target).
 *   res[k], caches[k], public_matrices[k]   key k, each as in gpupoly_trapdoor_preimage_many; all keys in one context,
 *                 at one level, with one d, and all caches with the same (sigma, s, dgg_stddev) - keys of one parameter set
 *   key_of[j], targets[j], outs[j]          request j; shapes, formats and tags as in gpupoly_trapdoor_preimage_many
 * Only the linear algebra and the perturbation's conditional Gaussians depend on the key, so the requests - ordered by
 * key (stable), cut into the same groups of up to 64 (p2 capped at 1 GiB; a boundary may fall inside a key's requests) -
 * share that entry's sequence of launches: p2 and the G-sampler as they are, p1 by a form of its sampler that finds each
 * segment's covariance cache in a device table (from the context's allocator, filled by one staged copy, released
 * stream-ordered), the three products as one launch each that takes a left operand per column range.  The number of
 * launches of a group does not depend on the number of keys.  Enqueued on the context's stream; the host does not block.
 * A key may have no requests; zero-column requests give zero-column outputs; n = 0 launches nothing; nkeys = 1 gives
 * what gpupoly_trapdoor_preimage_many gives.
 * A refused call launches nothing and writes no output, not even a format tag; every condition is checked for every key
 * and every request before the first launch: everything gpupoly_trapdoor_preimage_many refuses, per key and per
 * request; a null array with nkeys > 0 or n > 0; nkeys = 0 with n > 0; key_of[j] >= nkeys; keys that differ in d, level
 * or context; an output that aliases any key's [R; E] or A, any target or another output.  Refused with "unsupported" in
 * the text - issue one gpupoly_trapdoor_preimage_many per key then: everything that entry answers so, and caches whose
 * three widths are not all equal.                                                                                    */
int gpupoly_trapdoor_preimage_keyed(const GpuMatrix *const *res, const GpuP1CovarianceCache *const *caches,
                                    const GpuMatrix *const *public_matrices, size_t nkeys, uint32_t base_bits,
                                    const uint32_t *key_of, const GpuMatrix *const *targets, size_t n,
                                    const GpuRngSeed *seeds, GpuMatrix *const *outs);
/* ---- the producer of those requests (extension).  The GGH15 LUT preprocessing asks for one preimage per LUT
 * row and column chunk (sample_lut_preimages_gpu, src/lookup/ggh15/pubkey_gpu.rs:540-640; CPU twin pubkey.rs:241-275,441-460)
 * and builds every target with build_lut_preimage_target_chunk_gpu (pubkey_gpu.rs:379-415): a slice, a large-scalar product,
 * a tag hash, a decomposed hash sample, two products with their adds and a mul_scalar - per row.
 *
 * Decomposed blocks: G^-1 of nblk independently seeded samples in one call.  Replaces the per-tag
 * sample_hash_decomposed_columns of pubkey_gpu.rs:398-407 (and :495-504, poly_encoding_gpu.rs:453-462) for callers that
 * hold many tags.  out is (src_rows * k) x (nblk * c), c = out->cols / nblk, k as for gpupoly_matrix_decompose_rows, and
 *   out = [D_0 | D_1 | ... | D_(nblk-1)],
 * D_t being, bit for bit, what gpupoly_matrix_sample_decomposed_window(seeds[t], base_bits, small, src_rows, full_ncol,
 * col_offset, row_start = 0) writes into a (src_rows * k) x c matrix: every block is the window [col_offset, col_offset + c)
 * of its own conceptual src_rows x full_ncol matrix, a polynomial's stream id its position there (row * full_ncol +
 * col_offset + local column).  `out` keeps the format it was created with, EVAL or COEFF.  The seeded-blocks sampler
 * (gpupoly_matrix_sample_distribution_blocks, whose table gains the window) writes the coefficients into scratch from the
 * context's allocator - no transform, no pack - and, G^-1 working column by column, ONE digit transform over the wide
 * scratch gives every block: sub-keys, samples, digits; no launch count depends on nblk.  `seeds` are read before the call
 * returns.  Enqueued on the context's stream; the host does not block.  An `out` without polynomials succeeds with nothing
 * launched and is tagged EVAL.
 * Overlap: the only matrix is `out`; nothing can overlap.
 * Refused, with nothing launched and `out` (contents AND tag) untouched, the message naming this entry: a null `out` or
 * `seeds`; nblk == 0 or above 2^20; an invalid dist_type; base_bits of 0 or >= 63; out->cols not a multiple of nblk; a window
 * past full_ncol; out->rows != src_rows * k; src_rows * full_ncol beyond the samplers' 48-bit stream ids.  Refused likewise
 * with "unsupported" in the text: the Gaussian distribution; a context created under MXX_HIP_RNG_COMPAT=reference.        */
int gpupoly_matrix_sample_decomposed_blocks(GpuMatrix *out, int dist_type, const GpuRngSeed *seeds, size_t nblk,
                                            uint32_t base_bits, int small, size_t src_rows, size_t full_ncol,
                                            size_t col_offset);
/* The same with seeds[t] = hash_seed_for_matrix(key, tag_t) derived on the device by one launch in front, as
 * gpupoly_matrix_sample_hash_blocks does: the seeds never reach the host.  Refused likewise, plus everything
 * gpupoly_hash_seeds refuses of `tags`.                                                                              */
int gpupoly_matrix_sample_hash_decomposed_blocks(GpuMatrix *out, int dist_type, const GpuHashTags *tags, size_t nblk,
                                                 uint32_t base_bits, int small, size_t src_rows, size_t full_ncol,
                                                 size_t col_offset);
/* The preimage targets of T LUT rows of ONE column chunk: replaces build_lut_preimage_target_chunk_gpu
 * (src/lookup/ggh15/pubkey_gpu.rs:379-415) for the rows of a wave (the loop body of :590-613); the outputs are the `targets`
 * of gpupoly_trapdoor_preimage_many.  With c = outs[0]->cols, c0 = col_start, m = d * k, k = dpt * (level + 1):
 *   outs[t] = W_id[:, c0..c0+c) + W_gy * G^-1(G_d[:, c0..c0+c) o y_t) + (W_v + idx_t * W_vx) * G^-1(U_t[:, c0..c0+c)),
 * U_t the d x m uniform matrix under hash_seed_for_matrix(key, tag_t), y_t and idx_t constant polynomials.
 *   w_identity, w_gy, w_v, w_vx   d x m, EVAL, one context and one level (it may be below the top)
 *   outs[t]      d x c, made by the caller, tagged EVAL on success
 *   y_words      host memory: T integers of words_per_y little-endian 64-bit words each, reduced mod every q_l
 *                (gpupoly_matrix_load_coeff_words's rule; from_elem_to_constant of the reference)
 *   idx          host memory: T row indices, reduced likewise (from_usize_to_constant)
 *   tags         T tags (GpuHashTags above), e.g. the DECIMAL form with prefix "ggh15_lut_v_idx_<lut_id>_"
 * Everything is exact arithmetic on canonical residues, so the result equals the reference's sequence - slice,
 * gpu_matrix_fill_gadget, gpu_matrix_mul_scalar, decompose, the decomposed hash sample, the products and adds - bit for
 * bit.  Column c0 + cc of G_d is (j, tw, e); its product with the constant y_t has one non-zero residue, whose digits are
 * constants, so the large-scalar term is sum_{e' < dpt} weight(t, cc, e') * W_gy[i, (j, tw, e')] in every limb, weight = digit
 * e' of (y_t mod q_tw) * B^e mod q_tw; and the constant idx_t commutes with the product.  The rows go in groups whose digit
 * scratch m x (Tg * c) stays under 1 GiB (gpupoly_trapdoor_preimage_many's rule for p2); per group: one staged copy of the
 * rows' table (output pointers, idx_t and y_t mod q_l), the decomposed-blocks sample [V_0 | V_1 | ...], ONE product of the
 * stacked [W_v; W_vx] (2d x m, copied once per call) against it, one kernel for the T*c*L*dpt weights, one combine kernel
 * that forms every word with one lazy accumulator (dpt + 1 products, reduced once) and writes it straight into its output.
 * The launches of a group do not depend on T: no per-row upload, launch or synchronisation.  Scratch comes from the context's
 * allocator and is released stream-ordered; the host does not block; PACKED24 operands are unpacked first; T = 0 succeeds
 * with nothing launched.
 * Overlap: an outs[t] must overlap no operand and no other output, row views included (the message contains "overlap").
 * Refused, with nothing launched and every output (residues AND tag) untouched, everything checked for every t before the
 * first launch, the message naming this entry: a null array with T > 0, a null operand or outs[t]; a context, level or
 * shape mismatch (operands d x m, outputs d x c); an operand not in EVAL form; col_start + c > m; outputs of different
 * widths; words_per_y == 0; base_bits of 0 or >= 63; everything gpupoly_hash_seeds refuses of `tags`; the overlaps above.
 * Refused likewise with "unsupported" in the text: a context created under MXX_HIP_RNG_COMPAT=reference.              */
int gpupoly_matrix_lut_targets(GpuMatrix *const *outs, size_t nrows_T, const GpuMatrix *w_identity, const GpuMatrix *w_gy,
                               const GpuMatrix *w_v, const GpuMatrix *w_vx, size_t col_start, uint32_t base_bits,
                               const uint64_t *y_words, size_t words_per_y, const uint64_t *idx, const GpuHashTags *tags);
/* Test instrument: the weights and the combine kernel of gpupoly_matrix_lut_targets alone, with [top; bottom] GIVEN -
 * `product` is 2d x (T * c), EVAL, row t's columns at t * c - instead of sampled and multiplied:
 *   outs[t] = W_id[:, c0..c0+c) + W_gy * G^-1(G_d[:, c0..c0+c) o y_t) + product[0..d, t*c..) + idx_t * product[d..2d, t*c..).
 * It lets a test reach the lazy accumulator's bound with operands no sampler produces (every residue q - 1).  One group
 * whatever T; arguments, overlap rule and refusals as above (`product` counts as an operand; no tags, any keying).     */
int gpupoly_matrix_lut_targets_combine(GpuMatrix *const *outs, size_t nrows_T, const GpuMatrix *w_identity,
                                       const GpuMatrix *w_gy, const GpuMatrix *product, size_t col_start, uint32_t base_bits,
                                       const uint64_t *y_words, size_t words_per_y, const uint64_t *idx);
/* ---- the same for the other lookup back end (extension).  The LWE public-lookup preprocessing
 * (sample_aux_matrices_gpu, src/lookup/lwe/pubkey_gpu.rs:397-520) asks for one preimage per LUT row and column chunk and
 * builds every target with build_adjusted_target_chunk (:193-222): a constant upload, gpu_matrix_mul_scalar over the whole of
 * G_d and a d x m subtraction for A_z - G_d o x, a gadget slice with its mul_scalar, the decomposed hash sample
 * (derive_k_low_chunk_for_slot, src/lookup/lwe/utils.rs:152-178), a product and two more subtractions - per row; the target
 * then goes alone into preimage_batched_sharded.
 *
 * The preimage targets of T LUT rows of ONE column chunk of one (gate, slot); the outputs are the `targets` of
 * gpupoly_trapdoor_preimage_many.  With c = outs[0]->cols, c0 = col_start, m = d * k, k = dpt * (level + 1):
 *   outs[t] = A_lt[:, c0..c0+c) - G_d[:, c0..c0+c) o y_t - (A_z - G_d o x_t) * G^-1(U_t[:, c0..c0+c))
 *           = A_lt[:, c0..c0+c) - G_d[:, c0..c0+c) o y_t - A_z * G^-1(U_t[:, c0..c0+c)) + x_t * U_t[:, c0..c0+c),
 * U_t the d x m uniform matrix under hash_seed_for_matrix(key, tag_t), x_t and y_t constant polynomials.
 *   a_z, a_lt    d x m, EVAL, one context and one level (it may be below the top)
 *   outs[t]      d x c, made by the caller, tagged EVAL on success
 *   y_words      host memory: T integers of words_per_y little-endian 64-bit words each, reduced mod every q_l
 *                (gpupoly_matrix_load_coeff_words's rule; from_elem_to_constant of the reference)
 *   x            host memory: T LUT inputs, reduced likewise (from_usize_to_constant)
 *   tags         T tags (GpuHashTags above); "LWE_R_G_<gate>_<lut>_<entry>_slot<slot>" carries its index in the middle,
 *                so callers send the TABLE form
 * Everything is exact arithmetic on canonical residues, so the result equals the reference's sequence bit for bit.  The
 * two lines are equal because G_d * G^-1(U) = U in every limb: the digits of a canonical residue, weighted by B^e mod q,
 * sum to that residue.  x_t * U_t is read off the digits the product needs anyway - limb l of its entry (i, cc) is
 * sum_{e < dpt} (x_t B^e mod q_l) * D_t[(i, l, e), cc] taken in limb l, which holds for the transformed digits by linearity -
 * and column c0 + cc = (j, tw, e) of G_d o y_t is (y_t mod q_tw) B^e mod q_tw in every slot of limb tw of row j, zero
 * elsewhere.  Nothing of size d x m is built per row and G is never filled.  The rows go in groups whose digit scratch
 * m x (Tg * c) stays under 1 GiB, at most 2^20 rows; per group: one staged copy of the rows' table (output pointers,
 * x_t B^e mod q_l, (y_t mod q_tw) B^e mod q_tw, computed on the host), the decomposed-blocks sample [D_0 | D_1 | ...], ONE
 * product of A_z - as it is, no copy - against it, one combine kernel that forms every word with one lazy accumulator
 * (dpt products and up to two negated addends on top of A_lt's word, reduced once, or every lazy window where the modulus
 * leaves room for fewer terms) and writes it straight into its output.  The launches of a group do not depend on T: no
 * per-row upload, launch or synchronisation.  Scratch comes from the context's allocator and is released stream-ordered;
 * the host does not block; PACKED24 operands are unpacked first; T = 0 succeeds with nothing launched.
 * Overlap: an outs[t] must overlap no operand and no other output, row views included (the message contains "overlap").
 * Refused, with nothing launched and every output (residues AND tag) untouched, everything checked for every t before the
 * first launch, the message naming this entry: a null array with T > 0, a null operand or outs[t]; a context, level or
 * shape mismatch (operands d x m, outputs d x c); an operand not in EVAL form; col_start + c > m; outputs of different
 * widths; words_per_y == 0; base_bits of 0 or >= 63; everything gpupoly_hash_seeds refuses of `tags`; the overlaps above.
 * Refused likewise with "unsupported" in the text: a context created under MXX_HIP_RNG_COMPAT=reference.              */
int gpupoly_matrix_lwe_targets(GpuMatrix *const *outs, size_t nrows_T, const GpuMatrix *a_z, const GpuMatrix *a_lt,
                               size_t col_start, uint32_t base_bits, const uint64_t *y_words, size_t words_per_y,
                               const uint64_t *x, const GpuHashTags *tags);
/* Test instrument: the combine kernel of gpupoly_matrix_lwe_targets alone, with the digits - `digits` is m x (T * c), EVAL,
 * row t's columns at t * c - and `product` = A_z * digits - d x (T * c), EVAL - GIVEN instead of sampled and multiplied:
 *   outs[t][i, cc] = A_lt[i, c0 + cc] - G_d[i, c0 + cc] o y_t - product[i, t*c + cc]
 *                    + (in limb l) sum_{e < dpt} (x_t B^e mod q_l) * digits[(i, l, e), t*c + cc].
 * It lets a test reach the lazy accumulator's bound with operands no sampler produces (every residue q - 1).  One group
 * whatever T; arguments, overlap rule and refusals as above (`digits` and `product` count as operands, digits m x (T * c),
 * product d x (T * c); no tags, any keying).                                                                            */
int gpupoly_matrix_lwe_targets_combine(GpuMatrix *const *outs, size_t nrows_T, const GpuMatrix *a_lt,
                                       const GpuMatrix *digits, const GpuMatrix *product, size_t col_start,
                                       uint32_t base_bits, const uint64_t *y_words, size_t words_per_y, const uint64_t *x);
/* ---- the commitment's public parameters (extension).  The Wee25 commitment samples one trapdoor preimage
 * per public-parameter index and column part (sample_public_params, src/commit/wee25.rs:494-758) and builds every target
 * on its own (:696-728): a compact-bytes reload of T_bottom's part, secret_size zero-fills, entry writes and
 * decompositions with a concat_rows (build_j_2m_block, :536-584), two products and a subtraction; the target then goes
 * alone into preimage.
 *
 * The preimage targets of T indices x P consecutive column parts; the outputs are the `targets` of
 * gpupoly_trapdoor_preimage_many.  With s = secret_size, k = dpt * (level + 1), m_g = s * k, m_b = t_bottom's rows:
 *   outs[t * P + p] = G_s * J(idx[t], part_start + p) - W_t * T_bottom[:, (part_start + p) * m_b .. (part_start + p + 1) * m_b)
 *                   = X(idx[t], part_start + p)       - W_t * T_bottom[:, (part_start + p) * m_b .. (part_start + p + 1) * m_b),
 * W_t the s x m_b uniform matrix under hash_seed_for_matrix(key, tag_t), J the row-wise concatenation of G^-1(row_i).
 *   t_bottom     m_b x C, EVAL, C a multiple of m_b, one context and one level (it may be below the top; k follows it)
 *   outs[t*P+p]  s x m_b, made by the caller, tagged EVAL on success
 *   idx          host memory: T indices, any 64-bit values (global columns beyond the window simply do not hit)
 *   tags         T tags (GpuHashTags above) naming W_t: "wee25_w_block_" followed by the index as 8 little-endian bytes is
 *                the INDEXED_LE64 form for a consecutive run.  The library does not tie tags[t] to idx[t]
 * Everything is exact arithmetic on canonical residues, so the result equals the reference's sequence bit for bit.  The
 * two lines are equal because G_s * G^-1(X) = X in every limb, so G_s * J is the matrix X whose row i is row_i itself, and
 * the index arithmetic of build_j_2m_block leaves one row non-zero: with bg = idx / m_g and rho = idx mod m_g, row
 * i* = rho / k holds g[kk] * g[s'], kk = rho mod k, at the global columns bg * k + s', s' < k.  For kk = (tw, e) and
 * s' = (tw', e') that is the constant 2^((e + e') * base_bits) mod q_tw in every slot of limb tw when tw == tw' and zero
 * otherwise.  G is never built and nothing is decomposed.  The blocks go in groups whose W scratch (Tg * s) x m_b stays
 * under 1 GiB, at most 2^20 blocks, split further by blocks or columns where the product's grid would not fit; per group:
 * the hash launch, the stacked block sample [W_0; W_1; ...], one staged copy of the table (output pointers, i*, bg * k and
 * kk per block, the L * dpt^2 constants computed on the host) and ONE register-tiled product of the stacked W against the
 * window of T_bottom - as it is, no copy - whose epilogue reduces, negates canonically (q - r, 0 stays 0), adds the
 * constant where it hits and stores every target word once, straight into its output.  The launches of a group depend on
 * neither T nor P: no per-target upload, launch or synchronisation.  Scratch comes from the context's allocator and is
 * released stream-ordered; the host does not block; PACKED24 operands are unpacked first; T = 0 or P = 0 succeeds with
 * nothing launched.
 * Overlap: an output must overlap neither an operand nor another output, row views included (the message contains
 * "overlap").
 * Refused, with nothing launched and every output (residues AND tag) untouched, everything checked for every output before
 * the first launch, the message naming this entry: a null array with T * P > 0, a null operand or output; a context,
 * level or shape mismatch (outputs s x m_b); an operand not in EVAL form; C % m_b != 0 or (part_start + P) * m_b > C;
 * secret_size == 0; base_bits of 0 or >= 63; T * P overflowing; everything gpupoly_hash_seeds refuses of `tags`; the
 * overlaps above.  Refused likewise with "unsupported" in the text: a context created under MXX_HIP_RNG_COMPAT=reference. */
int gpupoly_matrix_wee25_targets(GpuMatrix *const *outs, size_t nblocks_T, size_t nparts_P, const GpuMatrix *t_bottom,
                                 size_t part_start, size_t secret_size, uint32_t base_bits, const uint64_t *idx,
                                 const GpuHashTags *tags);
/* Test instrument: the product kernel of gpupoly_matrix_wee25_targets alone, with [W_0; W_1; ...] GIVEN as `w_stacked`,
 * (T * s) x m_b, EVAL, instead of sampled:
 *   outs[t * P + p] = X(idx[t], part_start + p) - w_stacked[t*s .. (t+1)*s, :] * T_bottom[:, part part_start + p].
 * It lets a test reach the lazy accumulator's bound with operands no sampler produces (every residue q - 1).  Arguments,
 * overlap rule and refusals as above (`w_stacked` counts as an operand; no tags, any keying).                            */
int gpupoly_matrix_wee25_targets_product(GpuMatrix *const *outs, size_t nblocks_T, size_t nparts_P, const GpuMatrix *w_stacked,
                                         const GpuMatrix *t_bottom, size_t part_start, size_t secret_size,
                                         uint32_t base_bits, const uint64_t *idx);
/* ---- the online side of the GGH15 lookup (extension).  The evaluator's build_public_lookup_output_chunk
 * (src/lookup/ggh15/encoding.rs:172-300; device path src/lookup/ggh15/poly_encoding_gpu.rs:338-567,686-1420, stage-1 /
 * stage-2 tasks of one product each) runs per slot and output chunk: it re-reads the five gate preimages, samples and
 * decomposes V up to three times and multiplies P * rhs before c_b0 * (...).  With d the secret size, k = dpt * (level + 1),
 * m_g = d * k, w = d * (k + 2), r the rows of an encoding vector (1 in the reference), c_b0_s r x w, c_in_s r x m_g, x_s the
 * slot's plaintext, (k_s, y_s) = plt.get(x_s), V_s = G^-1(U_s[:, chunk]) for the d x m_g uniform U_s under tag_s
 * ("ggh15_lut_v_idx_<lut>_<k_s>") and K_s the chunk of the LUT-row preimage lut_aux_<lut>_idx<k_s>:
 *   out_s[:, chunk] = (c_b0_s P_id)[:, chunk] + (c_b0_s P_gy) G^-1(G_d[:, chunk] o y_s)
 *                   + (c_b0_s P_v + x_s o (c_b0_s P_vx) + c_in_s G^-1(U_g)) V_s - (c_b0_s P_g1) K_s.
 * Everything is exact ring arithmetic on canonical residues, so this re-association of the reference's c_b0 * (P * rhs)
 * changes no bit.  STAGE 1 is the caller's, with the existing product entries: the S slots' c_b0 / c_in stacked into
 * (S r)-row left factors against P_id, P_gy, P_v, P_vx, P_g1 and G^-1(U_g), each read once per wave instead of once per
 * slot and chunk.
 *
 * STAGE 2 of the lookup for S slots of one gate and ONE output column chunk [col_start, col_start + c), c = outs[0]->cols.
 * mid_* are the stage-1 products, slot s in rows [s r, (s + 1) r):
 *   mid_identity, mid_gy, mid_v, mid_vx, mid_rand   (S r) x m_g, EVAL      mid_gate1   (S r) x w, EVAL
 *   lut_preimages[s]   w x c, EVAL (the stored column chunk of the slot's LUT-row preimage; the same matrix may be given
 *                      for several slots)        xs[s]   1 x 1, EVAL        outs[s]   r x c, made by the caller, tagged EVAL
 *   y_words / tags     as gpupoly_matrix_lut_targets (y_s reduced mod every q_l; tag_s names U_s)
 * The slots go in groups whose scratch - the digits m_g x (Sg c) and the left factor (Sg r) x (m_g + w) - stays under 1 GiB
 * (MXX_HIP_GGH15_LOOKUP_BUDGET=<bytes> overrides the cap), at most 2^20 slots.  Per group: ONE staged copy of the slots'
 * table (output, K_s and x_s pointers; the weights of the gy term, digit e' of (y_s mod q_tw) B^e mod q_tw per (s, cc, e'),
 * computed on the host), the decomposed-blocks hash sample [V_0 | V_1 | ...], ONE pre-pass kernel that writes
 * Lhs = [mid_v + x_s o mid_vx + mid_rand | neg(mid_gate1)] with canonical residues (neg(0) = 0), and ONE main kernel: every
 * output word is mid_identity's word + m_g terms against V_s + w terms against K_s, read in place through the table, + dpt
 * weighted words of mid_gy, in one lazy accumulator folded every lazy_terms terms wherever they fall, reduced once, written
 * once.  A lane holds a term's left words in registers for a tile of up to 4 chunk columns and 2 rows, 16 bytes per load
 * and store (one word where a limb vector is narrower).  Launches per group: the sampler's (those of
 * gpupoly_matrix_sample_hash_decomposed_blocks for Sg tags) + 2 kernels + 1 copy, whatever S - 7 kernels and 2 copies for
 * 48 slots as for 2 at n = 256, 3 x 51 bits, against 88 kernels and 20 copies of the per-slot sequence for 2 slots of one
 * chunk (tests/test_gpu_ggh15_lookup.py); the slot descriptors live in the device table, not in the kernel arguments.  Scratch comes from the context's allocator and is released
 * stream-ordered; the host does not block; PACKED24 operands are unpacked first; S = 0 and c = 0 succeed with nothing
 * launched.
 * Overlap: an outs[s] must overlap no mid_*, no lut_preimages[t], no xs[t] and no other output, row views included (the
 * message contains "overlap").
 * Refused, with nothing launched and every output (residues AND tag) untouched, everything checked for every slot before
 * the first launch, the message naming this entry: a null array or entry; a context, level or shape mismatch; (S r) not
 * divisible by S; an operand not in EVAL form; col_start + c > m_g; outputs of different widths; words_per_y == 0;
 * base_bits of 0 or >= 63; everything gpupoly_hash_seeds refuses of `tags`; the overlaps above.  Refused likewise with
 * "unsupported" in the text: a context created under MXX_HIP_RNG_COMPAT=reference.                                       */
int gpupoly_matrix_ggh15_lookup(GpuMatrix *const *outs, size_t nslots_S, const GpuMatrix *mid_identity,
                                const GpuMatrix *mid_gy, const GpuMatrix *mid_v, const GpuMatrix *mid_vx,
                                const GpuMatrix *mid_rand, const GpuMatrix *mid_gate1,
                                const GpuMatrix *const *lut_preimages, const GpuMatrix *const *xs, size_t col_start,
                                uint32_t base_bits, const uint64_t *y_words, size_t words_per_y, const GpuHashTags *tags);
/* Test instrument: the same with the digits GIVEN - `digits` is m_g x (S * c), EVAL, slot s at columns [s c, (s + 1) c) -
 * instead of sampled: the table copy, the pre-pass and the main kernel alone, one group whatever S.  It lets a test reach
 * the lazy accumulator's bound with operands no sampler produces.  Arguments, overlap rule and refusals as above (`digits`
 * counts as an operand; no tags, any RNG keying).                                                                        */
int gpupoly_matrix_ggh15_lookup_combine(GpuMatrix *const *outs, size_t nslots_S, const GpuMatrix *mid_identity,
                                        const GpuMatrix *mid_gy, const GpuMatrix *mid_v, const GpuMatrix *mid_vx,
                                        const GpuMatrix *mid_rand, const GpuMatrix *mid_gate1,
                                        const GpuMatrix *const *lut_preimages, const GpuMatrix *const *xs, size_t col_start,
                                        uint32_t base_bits, const uint64_t *y_words, size_t words_per_y,
                                        const GpuMatrix *digits);
/* ---- the online side of the LWE lookup (extension).  The evaluator's public_lookup_poly_gpu
 * (src/lookup/lwe/poly_encoding_gpu.rs:419-453) is a plain loop over the slots, with a TODO asking for a slot-level
 * scheduler, around public_lookup_slot_gpu (src/lookup/lwe/encoding_gpu.rs:225-370), which per slot and column chunk forms
 * two products - c_b against the stored K_high chunk, the input vector against the decomposed hash sample K_low
 * (compute_wave, src/lookup/lwe/encoding_gpu.rs:142-188) -, takes both through compact bytes, concatenates the chunks and
 * adds the two families (reduce_contribution_bytes_by_chunk, :190-223).  With d the secret size, k = dpt * (level + 1),
 * m_g = d * k, w the rows of a stored K_high chunk (the width of the trapdoor's public matrix; not tied to d here) and r the
 * rows of an encoding vector (1 in the reference), this entry serves S slots of one gate and ONE output column chunk
 * [col_start, col_start + c), c = k_highs[0]->cols:
 *   out_s[:, dst_col .. dst_col + c) = c_b_s K_high_s + c_z_s G^-1(U_s[:, col_start .. col_start + c)),
 *   c_bs[s]   r x w, EVAL        k_highs[s]   w x c, EVAL (the stored chunk of the slot's LUT-row preimage)
 *   c_zs[s]   r x m_g, EVAL (m_g = c_zs[0]->cols, a multiple of k)        outs[s]   r x C, made by the caller, dst_col + c <= C
 *   U_s the d x m_g uniform matrix under hash_seed_for_matrix(key, tag_s), tag_s = "LWE_R_G_<gate>_<lut>_<entry_s>_slot<slot>":
 *   the entry index stands in the middle of the tag, so callers send the TABLE form of `tags`.
 * The same matrix may be given for several slots in c_bs, k_highs and c_zs; one context and one level, which may be below the
 * top.  Exact arithmetic on canonical residues: the result equals the reference's two gpu_matrix_mul, one gpu_matrix_add and
 * a copy_block into place bit for bit.  Columns of outs[s] outside the block are not touched; every output is tagged EVAL on
 * success, and a partial block into an output not already tagged EVAL is refused (gpupoly_matrix_mul_sum's rule), so a caller
 * writes every chunk straight into the full-width r x m_g result, without a concatenation.
 * The slots go in groups whose digit scratch m_g x (Sg c) stays under 1 GiB (MXX_HIP_LWE_LOOKUP_BUDGET=<bytes> overrides the
 * cap), at most 2^20 slots each.  Per group: ONE staged copy of the slots' table (output, c_b, K_high and c_z pointers), the
 * decomposed-blocks hash sample [D_0 | D_1 | ...] into scratch of the context's allocator, and ONE main kernel - no pre-pass,
 * the left factors are read in place through the table: every output word is one lazy accumulator over the w terms against
 * K_high_s and the m_g terms against D_s, folded every lazy_terms terms wherever they fall, reduced once and stored once.  A
 * lane holds a term's left words in registers for a tile of up to 4 chunk columns and 2 rows, 16 bytes per load and store
 * (one word where a limb vector is narrower); every word of K_high_s and D_s is loaded by one tile only.  Launches per group:
 * those of gpupoly_matrix_sample_hash_decomposed_blocks for Sg tags + 1 kernel + 1 copy, whatever S; the slot descriptors
 * live in the device table, not in the kernel arguments.  Scratch is released stream-ordered; the host does not block;
 * PACKED24 operands are unpacked first; S = 0, c = 0 and r = 0 succeed with nothing launched; w = 0 is legal and gives the
 * digits term alone.
 * Overlap: an outs[s] must overlap no c_bs[t], k_highs[t], c_zs[t] and no other output, row views included; disjoint views
 * of one parent are accepted (the message contains "overlap").
 * Refused, with nothing launched and every output (residues AND tag) untouched, everything checked for every slot before
 * the first launch, the message naming this entry: a null array or entry; a context, level or shape mismatch (the slot in
 * the message); an operand not in EVAL form; m_g not a multiple of k; col_start + c > m_g; dst_col + c > C; K_high chunks or
 * outputs of different widths; a partial block into a non-EVAL output; base_bits of 0 or >= 63; everything
 * gpupoly_hash_seeds refuses of `tags`; the overlaps above.  Refused likewise with "unsupported" in the text: a context
 * created under MXX_HIP_RNG_COMPAT=reference.                                                                            */
int gpupoly_matrix_lwe_lookup(GpuMatrix *const *outs, size_t nslots_S, size_t dst_col, const GpuMatrix *const *c_bs,
                              const GpuMatrix *const *k_highs, const GpuMatrix *const *c_zs, size_t col_start,
                              uint32_t base_bits, const GpuHashTags *tags);
/* Test instrument: the same with the digits GIVEN - `digits` is m_g x (S * c), EVAL, slot s at columns [s c, (s + 1) c) -
 * instead of sampled: the table copy and the main kernel alone, one group whatever S.  It lets a test reach the lazy
 * accumulator's bound with operands no sampler produces.  Arguments, overlap rule and refusals as above (`digits` counts as
 * an operand; no tags, any RNG keying).                                                                                  */
int gpupoly_matrix_lwe_lookup_combine(GpuMatrix *const *outs, size_t nslots_S, size_t dst_col,
                                      const GpuMatrix *const *c_bs, const GpuMatrix *const *k_highs,
                                      const GpuMatrix *const *c_zs, size_t col_start, uint32_t base_bits,
                                      const GpuMatrix *digits);
/* ---- the online side of the slot-transfer gates (extension).  The evaluator's output_slot_for_params
 * (src/slot_transfer/bgg_poly_encoding.rs:119-248) and slot_reduce_output_slot_for_params (:250-386) - on the device
 * src/slot_transfer/bgg_poly_encoding_gpu.rs:255-786: stage-1 tasks, stage-2 tasks, reduce_slot_transfer_matrix_bytes, all
 * behind the plain `for dst_slot` loop of evaluate_slot_transfer_slots_gpu (:748-786) - form per destination slot and column
 * chunk one one-row product per term and family (lhs * &rhs_chunk, :477 and :640), take each through compact bytes and
 * concatenate; c_b0 P0_src is recomputed for every destination, in slot_reduce num_slots times per destination (:300-372).
 * With d the secret size, k = dpt * (level + 1), m_g = d * k, r the rows of an encoding vector (1 in the reference), w0 the
 * columns of B0 and w1 the columns of B1 (d (k + 2) and 2 d (k + 2) in the reference; neither is tied to d here), a
 * destination slot s with terms t has
 *   out_s = c_b0 Pg_s + sum_t x^shift_t o kappa_t o ( c_in_t G^-1(A_s) + mu_t o ((c_b0 P0_src_t) P1_s) ),
 * Pg_s the stored gate preimage (w0 x m_g), P0_src (w0 x w1) and P1_s (w1 x m_g) the stored slot preimages, A_s the d x m_g
 * uniform matrix under hash_seed_for_matrix(key, "slot_transfer_slot_a_<s>"), mu_t the constant coefficient of the source
 * plaintext (an integer below Q), kappa_t the optional scalar; slot_transfer has one term per output with shift 0,
 * slot_reduce num_slots terms with shift = the source index and kappa = 1.  Exact arithmetic on canonical residues, so
 * re-associating changes no bit.  STAGE 1 is the caller's, with the product entries: mid_src = c_b0 P0_src once per DISTINCT
 * source.  STAGE 2, this entry, for S outputs of one gate and ONE output column chunk [col_start, col_start + c),
 * c = gate_preimages[0]->cols:
 *   LhsA_s = sum_t (kappa_t x^shift_t) o c_in_t (r x m_g)        LhsB_s = sum_t (kappa_t mu_t x^shift_t) o mid_t (r x w1)
 *   outs[s][:, dst_col .. dst_col + c) = c_b0 Pg_s[:, chunk] + LhsA_s G^-1(A_s[:, chunk]) + LhsB_s P1_s[:, chunk]
 *   c_b0   r x w0, EVAL        gate_preimages[s]   w0 x c, EVAL        b1_preimages[s]   w1 x c, EVAL
 *   terms of output s: terms[term_offsets[s] .. term_offsets[s + 1]), at least one; term_offsets has S + 1 entries from 0
 *   mu_words   one integer of words_per_mu little-endian 64-bit words PER TERM (as y_words of gpupoly_matrix_lut_targets)
 *   tags       tag_s names A_s: indexed-decimal form for consecutive destinations, the TABLE form otherwise
 *   outs[s]    r x C, made by the caller, dst_col + c <= C; columns outside the block are not touched
 * The same matrix may serve several outputs or terms.  Every output is tagged EVAL on success; a partial block into an
 * output not already EVAL is refused (gpupoly_matrix_mul_sum's rule), so a caller writes every chunk straight into the
 * full-width r x m_g result.
 * The outputs go in groups whose scratch - the digits m_g x (Sg c) and the left factors (Sg r) x (m_g + w1) - stays under
 * 1 GiB (MXX_HIP_SLOT_EVAL_BUDGET=<bytes> overrides the cap), at most 2^20 outputs each.  Per group: ONE staged copy of the
 * table (per output the output, Pg, P1 and A-segment pointers and the term range; per term the c_in and mid pointers, the
 * shift mod 2N and per limb kappa mod q_l and kappa mu mod q_l, computed on the host), the decomposed-blocks hash sample
 * [D_0 | D_1 | ...], ONE pre-pass kernel that writes LhsA and LhsB with canonical residues (a thread owns a 16-byte vector
 * of evaluation slots of 4 polynomials of one limb, forms weight * psi_l^(shift (2 bitrev(k) + 1)) once per term - no table
 * gather when the shift is 0 - and accumulates lazily), and ONE main kernel: gpupoly_matrix_lwe_lookup's register tile (up
 * to 2 rows x 4 chunk columns, 16 bytes per load and store, one word where a limb vector is narrower) with three streams
 * into one lazy accumulator - w0 terms of c_b0 against Pg_s, m_g terms of the A segment against D_s, w1 terms of LhsB_s
 * against P1_s - folded every lazy_terms terms wherever they fall, reduced once, stored once.  An output whose only term
 * has shift 0 (mod 2N) and scalar 1 gets no A segment: the main kernel reads its c_in in place.  Launches per group: those
 * of gpupoly_matrix_sample_hash_decomposed_blocks for Sg tags + 2 kernels + 1 copy, whatever S and the number of terms.
 * Scratch is released stream-ordered; the host does not block; PACKED24 operands are unpacked first; S = 0, c = 0 and
 * r = 0 succeed with nothing launched; w0 = 0 and w1 = 0 are legal; scalar = 0 is a legal weight.
 * Overlap: an outs[s] must overlap no operand and no other output, row views included; disjoint views of one parent are
 * accepted (the message contains "overlap").
 * Refused, with nothing launched and every output (residues AND tag) untouched, everything checked for every output and
 * term before the first launch, the message naming this entry and the slot or term: a null array or entry; a context,
 * level or shape mismatch; an operand not in EVAL form; term_offsets not non-decreasing from 0 or an output without terms;
 * m_g not a multiple of k; col_start + c > m_g; dst_col + c > C; preimage chunks or outputs of different widths; a
 * partial block into a non-EVAL output; words_per_mu == 0; base_bits of 0 or >= 63; everything gpupoly_hash_seeds refuses
 * of `tags`; the overlaps above.  Refused likewise with "unsupported" in the text: a context created under
 * MXX_HIP_RNG_COMPAT=reference.                                                                                          */
typedef struct {
    const GpuMatrix *c_in; /* r x m_g, EVAL */
    const GpuMatrix *mid;  /* r x w1, EVAL: c_b0 * P0_src, made by the caller (stage 1) */
    uint64_t shift;        /* the term is multiplied by x^shift, taken mod 2N */
    uint64_t scalar;       /* and by this integer; 1 = none */
} GpuSlotTerm;
int gpupoly_matrix_slot_transfer_eval(GpuMatrix *const *outs, size_t nouts_S, size_t dst_col, const GpuMatrix *c_b0,
                                      const GpuMatrix *const *gate_preimages, const GpuMatrix *const *b1_preimages,
                                      const GpuSlotTerm *terms, const size_t *term_offsets, const uint64_t *mu_words,
                                      size_t words_per_mu, size_t col_start, uint32_t base_bits, const GpuHashTags *tags);
/* Test instrument (the stage-2 tasks of src/slot_transfer/bgg_poly_encoding_gpu.rs:255-786 without their sampler): the
 * same with the digits GIVEN - `digits` is m_g x (S * c), EVAL, output s at columns [s c, (s + 1) c) - instead of sampled:
 * the table copy, the pre-pass and the main kernel alone, one group whatever S.  It lets a test reach the lazy
 * accumulator's bound with operands no sampler produces.  Arguments, overlap rule and refusals as above (`digits` counts as
 * an operand; no tags, any RNG keying).                                                                                  */
int gpupoly_matrix_slot_transfer_eval_combine(GpuMatrix *const *outs, size_t nouts_S, size_t dst_col, const GpuMatrix *c_b0,
                                              const GpuMatrix *const *gate_preimages,
                                              const GpuMatrix *const *b1_preimages, const GpuSlotTerm *terms,
                                              const size_t *term_offsets, const uint64_t *mu_words, size_t words_per_mu,
                                              size_t col_start, uint32_t base_bits, const GpuMatrix *digits);
/* ---- BGG+ encodings for many slots (extension).  BGGPolyEncodingSampler::sample
 * (src/bgg/sampler.rs:224-364; on the device src/bgg/sampler_gpu.rs:81-172) is a plain loop over the slots that per slot
 * (src/bgg/sampler_gpu.rs:110-160) loads the slot's secret mask from compact bytes, forms t = s S_slot, samples a fresh
 * Gaussian 1 x P m error, builds the plaintext row (from_poly_vec_row), multiplies t A_all, multiplies t G against a fully
 * filled gadget, takes the tensor product with the plaintexts, subtracts, adds, slices the row into P vectors and stores
 * compact bytes; BGGEncodingSampler::sample (src/bgg/sampler.rs:133-182) is the same sequence for one slot with t = s.  With
 * d the secret size, k = dpt * (level + 1), dpt = ceil(crt_bits / base_bits), m = d * k and P = 1 + the number of plaintexts:
 *   outs[i][sigma, :] = t_sigma A_i  -  pt[sigma][i] o (t_sigma G)  +  e_sigma[:, i m .. (i + 1) m),   i < P,  pt[sigma][0] = 1,
 *   secrets      S x d, EVAL: row sigma is t_sigma (the plain encoding sampler: S = 1 and the row is s itself)
 *   pubkeys[i]   d x m, EVAL; the same matrix may stand for several inputs
 *   plaintexts   S x (P - 1), EVAL, entry (sigma, i - 1) input i's plaintext in slot sigma; NULL exactly when P == 1
 *   outs[i]      S x m, made by the caller; tagged EVAL on success
 *   sigma == 0: no error, nothing is sampled, `seeds` may be NULL; sigma > 0: e_sigma is, bit for bit, what
 *   gpu_matrix_sample_distribution(GPU_MATRIX_DIST_GAUSS, sigma, seeds[sigma]) writes into a 1 x P m matrix.
 * (t G)[c] is t[c / k] times a constant that is non-zero in the one limb tower(c), where it is (2^base_bits)^e mod q
 * (gpupoly_matrix_mul_gadget's weights), so every output word is ONE lazy accumulator: the error residue (or 0) first, the
 * d products, and - in the limb the gadget hits, decided per workgroup - the term (q - pt t mod q) w; folded every lazy_terms
 * terms wherever they fall, reduced once, stored once.  Exact arithmetic on canonical residues: the result equals the
 * reference's sequence bit for bit.  One context and one level, which may be below the top.
 * The slots go in groups whose scratch - per slot the error row 1 x P m and the int64 samples staged for it - stays under
 * 1 GiB (MXX_HIP_BGG_ENCODE_BUDGET=<bytes> overrides the cap).  Per group: the launches of gpupoly_matrix_sample_gauss_blocks
 * for Sg seeds (STACKED layout, into scratch of the context's allocator), ONE staged copy of the table (the outs and pubkeys
 * pointers, the gadget weights) and ONE main kernel, whatever S and P; with sigma == 0 one copy and one kernel.  A lane owns
 * up to 4 slots x one column of one input in one limb, 16 bytes per load and store (one word where a limb vector is
 * narrower), and loads the d words of A_i[., c] once for the tile's slots.  Scratch is released stream-ordered; the host
 * does not block; PACKED24 operands are unpacked first; P = 0, S = 0, d = 0 and m = 0 succeed with nothing launched.
 * Overlap: an outs[i] must overlap no operand and no other output, row views included; disjoint views of one parent are
 * accepted (the message contains "overlap").
 * Refused, with nothing launched and every output (residues AND tag) untouched, everything checked before the first launch,
 * the message naming this entry: a null array or entry; plaintexts NULL with P > 1 or given with P == 1; a context, level or
 * shape mismatch (the input in the message); an operand not in EVAL form; m != d k; base_bits of 0 or >= 63; a sigma that is
 * negative or not finite; seeds NULL with sigma > 0; S > 2^20; the overlaps above.  Refused likewise with "unsupported" in
 * the text, as the Gaussian block sampler refuses them, and judged after everything above so that a mistake in the
 * operands is named first: sigma > 0 on a ring of n < 128, and sigma > 0 on a context created under
 * MXX_HIP_RNG_COMPAT=reference.  The outputs are tagged once the last group has been enqueued: a call that fails after its
 * checks (an allocation, a launch) returns non-zero and leaves the tags as they were.                                    */
int gpupoly_matrix_bgg_encode_slots(GpuMatrix *const *outs, size_t ninputs_P, const GpuMatrix *secrets,
                                    const GpuMatrix *const *pubkeys, const GpuMatrix *plaintexts, uint32_t base_bits,
                                    double sigma, const GpuRngSeed *seeds);
/* Test instrument, and the mirror's path where the block sampler is "unsupported": the same with the errors GIVEN -
 * `errors` is S x (P * m), EVAL, or NULL for none - instead of sampled: the table copy and the main kernel alone, one group
 * whatever S.  It lets a test reach the lazy accumulator's bound with errors no sampler produces.  Arguments, overlap rule
 * and refusals as above (`errors` counts as an operand; no sigma, no seeds, any ring and any RNG keying).                */
int gpupoly_matrix_bgg_encode_slots_combine(GpuMatrix *const *outs, size_t ninputs_P, const GpuMatrix *secrets,
                                            const GpuMatrix *const *pubkeys, const GpuMatrix *plaintexts,
                                            uint32_t base_bits, const GpuMatrix *errors);
/* ---- the message stream of the commitment-based lookup (extension).  The commit evaluator's stream
 * (build_msg_stream_for_lut_eval, src/lookup/commit_eval.rs:417-522) holds one d x m_b message block per LUT row of every
 * lookup gate and builds each on its own (:461-517): two hash samples, a gadget fill with a mul_scalar, a zero fill and a
 * concat_columns, a d x m_b * m_b x m_b product, a constant upload with a mul_scalar, a decomposition, a d x m_g * m_g x m_b
 * product and three additions or subtractions - per row, again in setup, commit_all_lut_matrices and every public_lookup.
 *
 * The message blocks of T LUT rows of `ngates` gates.  With d the secret size, k = dpt * (level + 1), m_g = d * k,
 * m_b = d * (k + 2), g = gate_of_row[t]:
 *   R_t        = the d x m_b uniform matrix under hash_seed_for_matrix(key, tag_t)
 *   canceler_t = (b_1 * V_t + R_t) o iota_t,    V_t = verifier[:, vslot[t] * m_b .. (vslot[t] + 1) * m_b),
 *                                               iota_t = (idx[t] + 1)^-1 mod q_l in limb l
 *   outs[t]    = [ a_outs[g] - G_d o y_t | 0_{d x (m_b - m_g)} ] + R_t - pubkey_sums[g] * G^-1(canceler_t),
 * y_t a constant polynomial.
 *   outs[t]          d x m_b, made by the caller, tagged EVAL on success
 *   b_1              d x m_b, EVAL
 *   verifier         m_b x (nV * m_b), EVAL, any nV >= 1; the library does not tie vslot[t] to idx[t]
 *   pubkey_sums[g]   d x m_g, EVAL: A_in,g + A_one,g
 *   a_outs[g]        d x m_g, EVAL
 *   gate_of_row      host memory: T gate numbers below ngates
 *   y_words          host memory: T integers of words_per_y little-endian 64-bit words each, reduced mod every q_l
 *                    (gpupoly_matrix_load_coeff_words's rule; from_elem_to_constant of the reference)
 *   idx              host memory: T LUT row indices
 *   tags             T tags (GpuHashTags above) naming R_t: "R_<g>_" followed by the decimal index is the INDEXED_DECIMAL
 *                    form for a consecutive run of one gate.  The library does not tie tags[t] to idx[t]
 * One context and one level (it may be below the top; k follows it).  Everything is exact arithmetic on canonical residues,
 * so the result equals the reference's sequence bit for bit.  Column (j, tw, e) of G_d o y_t is (y_t mod q_tw) B^e mod q_tw in
 * every slot of limb tw of row j and zero elsewhere; G is never filled.  One product of b_1 - as it is, no copy - against
 * the verifier gives every b_1 * V_t of the call.  The rows go in groups whose digit scratch m_g x (Tg * m_b) stays under
 * 1 GiB, at most 2^20 rows (MXX_HIP_COMMIT_LUT_BUDGET=<bytes> lowers the cap); per group: one staged copy of the rows' table
 * (output and operand pointers, vslot, iota_t mod q_l and (y_t mod q_tw) B^e mod q_tw, computed on the host), the stacked
 * block sample [R_0 | R_1 | ...], one elementwise kernel C[:, t-th block] = (BV[:, vslot_t block] + R_t) o iota_t, the
 * decomposition of the d x (Tg * m_b) matrix C (inverse transform, digits, forward transforms), and ONE register-tiled
 * product whose left operand is chosen per row - pubkey_sums[g] read in place - and whose epilogue negates the reduced sum
 * canonically (q - r, 0 stays 0), adds R_t's word and, in columns below m_g, a_outs[g]'s word and the negated gadget constant
 * in the one limb and row where it is non-zero, and stores every word once, straight into outs[t]; where the modulus leaves
 * room for fewer terms the sums are reduced in every lazy window.  The launches of a group depend on neither T nor ngates:
 * no per-row upload, launch or synchronisation.  Scratch comes from the context's allocator and is released stream-ordered;
 * the host does not block; PACKED24 operands are unpacked first; T = 0 succeeds with nothing launched.
 * Overlap: an outs[t] must overlap no operand and no other output, row views included (the message contains "overlap").
 * Refused, with nothing launched and every output (residues AND tag) untouched, everything checked for every t before the
 * first launch, the message naming this entry: a null array with T > 0, a null operand or outs[t]; ngates == 0 with T > 0;
 * gate_of_row[t] >= ngates; vslot[t] >= nV; a verifier whose column count is not a positive multiple of its row count; a
 * context, level or shape mismatch (b_1 and outputs d x m_b, verifier m_b rows, per-gate operands d x m_g); an operand not
 * in EVAL form; words_per_y == 0; base_bits of 0 or >= 63; idx[t] + 1 = 0 mod q_l for some limb (no inverse; the message
 * names the row); everything gpupoly_hash_seeds refuses of `tags`; the overlaps above.  Refused likewise with "unsupported"
 * in the text: a context created under MXX_HIP_RNG_COMPAT=reference.                                                   */
int gpupoly_matrix_commit_lut_messages(GpuMatrix *const *outs, size_t nrows_T, const GpuMatrix *b_1, const GpuMatrix *verifier,
                                       const uint64_t *vslot, const GpuMatrix *const *pubkey_sums,
                                       const GpuMatrix *const *a_outs, size_t ngates, const uint32_t *gate_of_row,
                                       uint32_t base_bits, const uint64_t *y_words, size_t words_per_y, const uint64_t *idx,
                                       const GpuHashTags *tags);
/* Test instrument: the combine kernel of gpupoly_matrix_commit_lut_messages alone, with [R_0 | R_1 | ...] - `r_stacked` is
 * d x (T * m_b), EVAL, row t's columns at t * m_b - and the digits - `digits` is m_g x (T * m_b), EVAL, likewise - GIVEN
 * instead of sampled, multiplied and decomposed:
 *   outs[t] = [ a_outs[g] - G_d o y_t | 0 ] + r_stacked[:, t*m_b .. (t+1)*m_b) - pubkey_sums[g] * digits[:, t*m_b .. (t+1)*m_b).
 * It lets a test reach the lazy accumulator's bound with operands no sampler produces (every residue q - 1).  One group
 * whatever T; arguments, overlap rule and refusals as above (`r_stacked` and `digits` count as operands; no verifier, vslot,
 * idx or tags, any keying).                                                                                            */
int gpupoly_matrix_commit_lut_messages_combine(GpuMatrix *const *outs, size_t nrows_T, const GpuMatrix *r_stacked,
                                               const GpuMatrix *digits, const GpuMatrix *const *pubkey_sums,
                                               const GpuMatrix *const *a_outs, size_t ngates, const uint32_t *gate_of_row,
                                               uint32_t base_bits, const uint64_t *y_words, size_t words_per_y);
/* Exact scale-and-round of every coefficient (extension): coefficient k of out[i][j] becomes
 *   floor((t * c + h) / Q) mod t,   h = round_half ? floor(Q/2) : 0,
 * c the coefficient of in[i][j] as coeffs() gives it (in [0, Q)), Q the context's FULL modulus; written as its residue
 * mod every limb of `out`, which is tagged COEFF on success.  round_half = 0 is modulus_switch
 * (src/matrix/gpu_dcrt_poly.rs:1352-1372, src/element/finite_ring.rs:22-26; the reference then re-NTTs through
 * from_coeffs / from_poly_vec), round_half = 1 the centred decode of decode_centered_masked_matrix
 * (src/decoder/masked_high_bit.rs:21-29,39-70; from_biguints / set_entry there).  One thread per coefficient: two Garner
 * passes and the exact quotient mod the prime 2^64 - 59, no floating point.  `in` may be COEFF or EVAL (an EVAL input is
 * inverse-transformed in `out`'s storage) and is left as it was unless out == in.  `out` has in's context and shape and
 * is at full level.  Enqueued on the context's stream; the host does not block.
 * Refused, with nothing launched and `out` (contents and tag) untouched: a null matrix, t = 0, a context, shape or
 * level mismatch.  Refused with an error containing "unsupported", likewise untouched: t >= 2^64 - 59, an input below
 * full level (rescale those on the host).                                                                         */
int gpupoly_matrix_scale_round(GpuMatrix *out, const GpuMatrix *in, uint64_t t, int round_half);
/* Rounded CRT recomposition of decoded level vectors in one call (extension): crt_recompose_rows
 * (src/noise_refresh/naive_vec.rs:2086-2118) and the combination of terms in front of it on the online path
 * (src/noise_refresh/naive_vec.rs:1654-1690).  With L the context's limb count, Q its full modulus and
 * T = terms_per_level in 1..8, `terms` holds num_slots * L * T matrices; terms[(slot * L + i) * T + t] is term t of
 * level (slot, i), signs[t] is +1 or -1 and is shared by every level, and level (slot, i) = sum_t signs[t] * term_t
 * mod Q.  T = 1 with sign +1 is the reference function; T = 4 with signs (+, +, -, -) is the online path's
 * `input_term + refresh_term - one_term - decoder` (:1687).  The result is
 *   out[slot][col] limb i, coefficient k = floor((q_i * c + floor(Q/2)) / Q) mod q_i,
 * c in [0, Q) coefficient k of entry col of level (slot, i): the centred decode for the plaintext modulus q_i
 * (decode_centered_masked_integer_coeff, src/decoder/masked_high_bit.rs:21-29).  That is the reference's
 * sum_i decode(level_i, q_i) * reconst_coeffs[i] exactly, because reconst_coeffs[i] (src/poly/mod.rs:45-60) is 1 mod
 * q_i and 0 mod every other limb.  Every term is 1 x c, at full level, on out's context, and all terms of a call have
 * one format (all COEFF or all EVAL); `out` is num_slots x c at full level, is written whole and tagged EVAL.  Terms may
 * repeat; no term is modified.  The signed sums go into scratch of the call (EVAL terms are summed as they lie, then one
 * inverse transform per level), one thread per output word runs the exact rounding of gpupoly_matrix_scale_round with
 * t = q_i, and one forward transform of `out` follows.  Scratch comes from the context's allocator, capped by
 * MXX_HIP_CRT_RECOMPOSE_CHUNK_BYTES (default 256 MiB, never less than one slot): the call works through whole slots per
 * chunk.  Enqueued on the context's stream; the host does not block.  c = 0 launches nothing and sets the tag.
 * Overlap: rule 3 - `out` must not overlap any term, row views included (the message contains "overlap").
 * Refused, before the first launch and with `out` (contents and tag) untouched, the message naming this entry: a null
 * `out`, `terms` or `signs`; a null terms[j]; num_slots = 0; T = 0 or T > 8; a sign other than +1 / -1; a context or
 * shape mismatch (`out` not num_slots x c, a term not 1 x c); terms of mixed formats; `out` not at full level; any
 * overlap of `out` with a term.  Refused likewise with an error containing "unsupported": a term below full level
 * (recompose those with the per-level calls).                                                                     */
int gpupoly_matrix_crt_recompose_rounded(GpuMatrix *out, const GpuMatrix *const *terms, const int *signs,
                                         size_t terms_per_level, size_t num_slots);
/* The nested-RNS gadget on the device (extension).  p_moduli are p_count pairwise coprime small integers
 * (sample_crt_primes, src/gadgets/arith/nested_rns/encoding.rs:14-71: 3, 4, 5, 7, 11, ... - not all prime), P their
 * product; the window is limbs level_offset .. level_offset + active_levels - 1 of the matrix's L limbs
 * (resolve_nested_rns_active_window, :146-160), Q_act their product, Q the product of all L.  With
 *   rdiv(a, b) = floor((a + floor(b/2)) / b),  inv_j = ((P/p_j) mod p_j)^-1 mod p_j,
 *   terms(x_0..): y_j = (x_j mod p_j) inv_j mod p_j, w = rdiv(sum_j rdiv(y_j scale, p_j), scale)            (:196-214)
 *   slot(a, x_0..) = ((sum_j y_j (P/p_j) - w P) rc_a) mod Q,  rc_a = (Q_act/q_a) ((Q_act/q_a) mod q_a)^-1    (:166-180,:222-238)
 * and slot(a, s) = slot(a, s mod p_0, ...) for an integer s, with D = p_count and A = active_levels:
 *
 * gpupoly_matrix_nested_rns_decompose is nested_rns_gadget_decomposed (:273-338; callers
 * src/gadgets/arith/nested_rns/poly.rs:1682-1693 and src/gadgets/fhe/ring_gsw_nested_rns.rs:33-92): `out` is
 * rows A (D+1) x cols for a rows x cols `src`; with r the residue of coefficient k of src[row][col] in limb
 * level_offset + a and (y, w) = terms(r mod p_0, ...), coefficient k of out[row A (D+1) + a (D+1) + d][col] is
 * slot(a, y_d) for d < D and slot(a, w) for d = D, as its residue in every limb (zero in the window's other limbs).
 * `src` may be COEFF or EVAL (an EVAL source is inverse-transformed in scratch of the call) and is never modified; `out`
 * is written whole and tagged out_format (GPU_POLY_FORMAT_EVAL: one forward transform at the end - over the full window
 * only of the one non-zero limb per row, in scratch, before it is spread over `out`).
 *
 * gpupoly_matrix_fill_nested_rns_gadget is nested_rns_gadget_vector (:240-271): `out` is 1 x A (D+1); every
 * coefficient of entry a (D+1) + d is slot(a, g), g = (P/p_d) mod q_a for d < D and (q_a - P mod q_a) mod q_a for d = D,
 * q_a limb level_offset + a.  Tagged out_format as the reference's from_biguints of n equal coefficients would be.
 *
 * gpupoly_matrix_nested_rns_residues is the first stage alone: out[row A D + a D + j][col] holds r mod p_j at
 * coefficient k, the same small integer in every limb - the slot-wise form of encode_nested_rns_poly_with_offset
 * (:401-420) that ciphertext_inputs_from_native (ring_gsw_nested_rns.rs:368-419) builds one coefficient at a time.
 * `out` is rows A D x cols and is tagged COEFF.
 *
 * The tables of a set of arguments (per-p reciprocals and look-ups, per-limb constants, slot(a, s) for every small s)
 * are built on the first call with it and kept by the context.  Enqueued on the context's stream; the host does not
 * block (but for that first build).  0 rows or 0 columns launch nothing and set the tag.
 * Overlap: rule 3 - `out` must not overlap `src`, row views included (the message contains "overlap").
 * Refused, with nothing launched and `out` (contents and tag) untouched, the message naming the entry: a null argument;
 * an out_format that is neither; a context, level or shape mismatch (`out` at src's level); active_levels = 0 or
 * level_offset + active_levels beyond the matrix's limbs; any overlap of `out` with `src`.  Refused likewise with an
 * error containing "unsupported": p_count outside 1..64, a p_j outside [2, 2^16), moduli that are not pairwise coprime,
 * scale = 0, (p_max - 1) scale + p_max/2 or p_count scale + scale/2 at or above 2^64.                             */
int gpupoly_matrix_nested_rns_decompose(GpuMatrix *out, const GpuMatrix *src, const uint64_t *p_moduli, size_t p_count,
                                        uint64_t scale, size_t level_offset, size_t active_levels, int out_format);
int gpupoly_matrix_fill_nested_rns_gadget(GpuMatrix *out, const uint64_t *p_moduli, size_t p_count, uint64_t scale,
                                          size_t level_offset, size_t active_levels, int out_format);
int gpupoly_matrix_nested_rns_residues(GpuMatrix *out, const GpuMatrix *src, const uint64_t *p_moduli, size_t p_count,
                                       size_t level_offset, size_t active_levels);
/* Every coefficient of `mat` as its value in [0, Q_level): little-endian 64-bit words, words_per_coeff words each
 * (zero above the words Q_level needs), order [row][col][k], into host memory `out` (synchronous).  COEFF or EVAL
 * input (an EVAL input is inverse-transformed in scratch; `mat` is left as it was).  Replaces the host CRT of
 * coeffs() / coeffs_biguints() (src/poly/dcrt/gpu.rs:959-994).  A words_per_coeff below what Q_level needs is
 * refused with nothing launched.                                                                                  */
int gpupoly_matrix_store_coeff_words(const GpuMatrix *mat, uint64_t *out, size_t words_per_coeff);
/* The way in (extension): coefficient k of entry (row, col) of `mat` becomes x mod q_l for every limb
 * l <= mat->level, x the integer that words_per_coeff little-endian 64-bit words spell; `words` is host memory in the
 * order [row][col][k][w], k < coeffs_per_poly, w < words_per_coeff - the mirror image of what
 * gpupoly_matrix_store_coeff_words writes.  x need not be below Q_level: every limb reduces the whole value, like the
 * BigUint % q of residues_from_biguints (src/poly/dcrt/gpu.rs:841-857), which this replaces together with the upload
 * and transform of from_biguints / from_coeffs (:903-939).  words_per_coeff may be smaller or larger than the words of
 * Q_level.  coeffs_per_poly <= N; coefficients at or above it are written as 0, so every word of `mat` is written
 * whatever it held (coeffs_per_poly = 0: the zero matrix, `words` may be null).  out_format GPU_POLY_FORMAT_COEFF leaves
 * the residues as loaded, GPU_POLY_FORMAT_EVAL runs the forward transform in place afterwards; `mat` is tagged with it on
 * success.  Synchronous: `words` may be reused on return.  0 rows or 0 columns succeed with nothing launched.
 * Refused, with nothing launched and `mat` (contents and tag) untouched: a null `mat`, null `words` with
 * coeffs_per_poly > 0, words_per_coeff = 0 or above 2^32 - 1, coeffs_per_poly > N, an out_format that is neither.    */
int gpupoly_matrix_load_coeff_words(GpuMatrix *mat, const uint64_t *words, size_t words_per_coeff, size_t coeffs_per_poly,
                                    int out_format);
/* Exact centred infinity norm of every entry: max_i |x_i| with x_i coefficient i of entry (row, col) taken in
 * (-Q_level/2, Q_level/2] - min(v, Q_level - v) for v in [0, Q_level) - as little-endian 64-bit words, words_per_value
 * words each (zero above the words Q_level needs), order [row][col], into host memory `out` (synchronous).  COEFF or EVAL
 * input (an EVAL input is inverse-transformed in scratch; `mat`'s residues and format are left as they were); 0 rows or
 * 0 columns succeed with nothing launched.  Replaces the host loops over coeffs() with min(v, Q - v) and a max: the
 * preimage predicate (src/sampler/trapdoor/gpu.rs:690-752, the p-hat form :756-812) and matrix_centered_max_abs
 * (tests/test_gpu_diamond_injector_q_bits_vs_max_error_plot_generates_svg.rs:145-163).  A null argument or a
 * words_per_value below what Q_level needs is refused with nothing launched and nothing written.                  */
int gpupoly_matrix_centered_max_abs(const GpuMatrix *mat, uint64_t *out, size_t words_per_value);
/* One bit per coefficient (extension): with c_k in [0, Q_level) coefficient k of entry (row, col), bit
 * k % 8 of byte out[(row * cols + col) * bytes_per_poly + k / 8] is set iff c_k lies in the interval that the bounds
 * `lo` and `hi` give - words_per_bound little-endian 64-bit words each, both in [0, Q_level] (Q_level itself allowed):
 *   lo <= hi: [lo, hi);   lo > hi: the wrap-around set [lo, Q_level) u [0, hi)  (|x| <= B in the centred
 *   representative is lo = Q_level - B, hi = B + 1);   lo == hi is the empty set, (0, Q_level) everything.
 * `out` is host memory (synchronous); every byte of every slot is written, bits at or above N and bytes at or above
 * ceil(N / 8) as zero.  COEFF or EVAL input (an EVAL input is inverse-transformed in scratch; `mat`'s residues and
 * format are left as they were); 0 rows or 0 columns succeed with nothing launched.  One thread per coefficient: Garner's
 * mixed-radix digits compared with the bounds' digits, top digit first - no big integer is built.  Replaces the host
 * loops over coeffs() of extract_bits_with_threshold (src/poly/dcrt/gpu.rs:1070-1081; lo = (Q/2) >> 1, hi = 3 lo) and of
 * the boolean centred decode (decode_centered_masked_boolean_coeff, src/decoder/masked_high_bit.rs:31-35;
 * lo = ceil((Q + 1) / 4), hi = ceil((3 Q + 1) / 4)).
 * Refused, with nothing launched and `out` untouched: a null argument, words_per_bound = 0, a bound above Q_level
 * (non-zero words above Q_level's words included), bytes_per_poly < ceil(N / 8).                                    */
int gpupoly_matrix_extract_bits(const GpuMatrix *mat, const uint64_t *lo, const uint64_t *hi, size_t words_per_bound,
                                uint8_t *out, size_t bytes_per_poly);
/* The first coeffs_per_poly (<= N) coefficients of every entry as machine integers (extension): elements
 * of elem_bytes (4 or 8) bytes, b = 8 * elem_bytes bits, order [row][col][k], into host memory `out` (synchronous).
 *   centred == 0: the element is c mod 2^b, c in [0, Q_level); it fits iff c < 2^b.
 *   centred != 0: the element is x mod 2^b (two's complement), x the representative of c in (-Q_level/2, Q_level/2];
 *                 it fits iff -2^(b-1) <= x <= 2^(b-1) - 1.
 * A coefficient that does not fit is still written, truncated as stated, and the call still returns 0:
 * *out_misfit_count is the number of such coefficients and *out_first_misfit the smallest linear index
 * (row * cols + col) * coeffs_per_poly + k among them, UINT64_MAX when there are none.  COEFF or EVAL input (an EVAL
 * input is inverse-transformed in scratch; `mat` is left as it was).  0 rows, 0 columns or coeffs_per_poly = 0 succeed
 * with nothing launched, count 0 and first UINT64_MAX.  Replaces the host loops over coeffs() of to_bool_vec
 * (src/poly/dcrt/gpu.rs:1083-1097) and coeffs_digits (src/poly/mod.rs:130-139), and the store + host CRT of
 * const_coeff_u64 (gpu.rs:1103-1120; coeffs_per_poly = 1).
 * Refused, with nothing launched and nothing written (both counters included): a null argument, elem_bytes other than
 * 4 or 8, coeffs_per_poly > N.                                                                                        */
int gpupoly_matrix_store_coeff_ints(const GpuMatrix *mat, void *out, int elem_bytes, int centred, size_t coeffs_per_poly,
                                    uint64_t *out_misfit_count, uint64_t *out_first_misfit);
/* The compact wire format for MANY matrices in one call (extension): what a loop over
 * gpu_matrix_store_compact_bytes / gpu_matrix_load_compact_bytes gives, with one width launch, one pack launch, one copy
 * of the widths, one copy of the payloads and two synchronises per CALL (up to 32 matrices of a level per launch)
 * instead of per matrix.  Replaces the per-matrix to_compact_bytes of get_lookup_buffer (src/storage/write.rs:724-793)
 * and the per-slot from_compact_bytes of the reading side (src/storage/read.rs:129-149).
 * Store: for every j < n the triple (out_max_coeff_bits[j], out_bytes_per_coeff[j], the out_payload_lens[j] bytes at
 * payload_out + out_payload_offsets[j]) is exactly what gpu_matrix_store_compact_bytes(mats[j], ...) reports and writes
 * for that matrix alone: every matrix keeps its OWN matrix-wide width.  out_payload_offsets[0] = 0, offsets are multiples
 * of 8 and do not decrease with j, the bytes between a payload's end and the next offset (at most 7) are zero,
 * *out_total_len = the last offset + the last length.  Like the one-matrix entry, an EVAL matrix is taken to the
 * coefficient domain in place (the caller records the tag beforehand); zero matrices and matrices without entries give
 * width 0 and length 0.  Synchronous: the bytes are in payload_out on return.  When payload_capacity < *out_total_len the
 * call fails with "payload buffer too small ..." AND fills all five out arrays / values, payload_out untouched, so that
 * the caller retries once with the exact size (the matrices are in COEFF form by then, as after the one-matrix entry).
 * Load: mats[j] receives what gpu_matrix_load_compact_bytes(mats[j], payloads[j], payload_lens[j], max_coeff_bits[j])
 * gives it, tagged COEFF.  The payloads are separate host pointers (in a lookup buffer a header sits in front of each).
 * Synchronous: the payloads may be freed on return.
 * One context per call; levels and shapes may differ from matrix to matrix; n = 0 does nothing.  Matrices whose
 * coefficients leave the two fast CRT forms, contexts above 16 limbs and MXX_HIP_SERDE=general go through the general
 * kernels one by one inside the same call (at most one further synchronise).
 * Refused, with nothing launched and every matrix (contents and tag) and every out value untouched: a null array with
 * n > 0, a null matrix, matrices of different contexts, the same matrix twice; for the load additionally everything the
 * one-matrix load refuses (length mismatch, non-zero length at width 0, null payload), checked for ALL j before the
 * first copy.                                                                                                      */
int gpupoly_matrix_store_compact_bytes_many(GpuMatrix *const *mats, size_t n, uint8_t *payload_out, size_t payload_capacity,
                                            uint16_t *out_max_coeff_bits, uint16_t *out_bytes_per_coeff,
                                            size_t *out_payload_offsets, size_t *out_payload_lens, size_t *out_total_len);
int gpupoly_matrix_load_compact_bytes_many(GpuMatrix *const *mats, size_t n, const uint8_t *const *payloads,
                                           const size_t *payload_lens, const uint16_t *max_coeff_bits);
/* Products by monomials on the device (extension).  Shifts are any uint64_t, taken as shift & (2N - 1):
 * x^N = -1 in Z_q[x] / (x^N + 1).  Every slot-packing step of the reference's callers is such a sum, one host loop
 * iteration per term: collapse_slot_matrices (src/noise_refresh/naive_vec.rs:1983-1998: sum_slot M_slot *
 * const_rotate_poly(slot), num_slots == ring_dim terms), the slot-transfer reduce step
 * (src/slot_transfer/bgg_poly_encoding.rs:362-380: c_gate + sum_src pre_slot_src * x^src), the target of slot_reduce on the
 * GPU path (src/slot_transfer/bgg_pubkey_gpu.rs:448-464: lhs_chunk - sum_src (...) * x^src) and rotate_gate /
 * monomial_scalar (src/circuit/poly_circuit/construction.rs:352-357, src/slot_transfer/bgg_poly_encoding.rs:706,942).  Per
 * term that loop builds a one-hot vector on the host, uploads and transforms it (from_u32s / from_coeffs;
 * const_rotate_poly, src/poly/mod.rs:151-156, goes through coeffs() - a host CRT of N big integers - first), then
 * gpu_matrix_mul_scalar and gpu_matrix_add: three launches, one upload, five passes over a matrix.
 *
 * gpupoly_matrix_fill_monomial: every entry of `out` becomes x^shift, written directly in `format` - COEFF: the one-hot
 * vector with +1 at coefficient shift mod N, or -1 (as q - 1 in every limb) when shift mod 2N >= N; EVAL: slot k of limb l
 * is psi_l^(shift (2 bitrev(k) + 1)), read from the context's forward twiddle table.  `out` is tagged with `format`.
 * Replaces const_rotate_poly and the from_u32s(one-hot) idiom.  Enqueued on the context's stream; 0 rows or 0 columns
 * succeed with nothing launched.  Refused, with nothing launched and `out` untouched: a null `out`, a `format` that is
 * neither GPU_POLY_FORMAT_COEFF nor GPU_POLY_FORMAT_EVAL.                                                              */
int gpupoly_matrix_fill_monomial(GpuMatrix *out, uint64_t shift, int format);
/* out = in * x^shift: gpupoly_matrix_monomial_sum with n = 1, no addend and negate = 0 - its semantics and refusals
 * (`out` must not overlap `in`; a null `out` or `in` is refused).                                                      */
int gpupoly_matrix_mul_monomial(GpuMatrix *out, const GpuMatrix *in, uint64_t shift);
/* out = addend + sgn * sum_{j<n} mats[j] * x^shifts[j],  sgn = negate ? -1 : +1.
 * One context, one level (it may be below the context's top level) and one shape for `out`, `addend` and every mats[j];
 * all of mats[j] and `addend` share one format, COEFF or EVAL, and `out` is tagged with it on success.  `addend` may be
 * NULL; out == addend accumulates in place (every word is read and written by the same thread).  The residues are, bit
 * for bit, those of the existing sequence - in EVAL gpupoly_matrix_fill_monomial, gpu_matrix_mul_scalar and gpu_matrix_add
 * / gpu_matrix_sub per term, in COEFF the inverse transform of that sequence on the transformed operands: everything is
 * exact modular arithmetic on canonical residues.  In EVAL each term is a point-wise product by the twiddle-table entry
 * psi^(shift (2 bitrev(k) + 1)), accumulated lazily; in COEFF a signed rotation: coefficient i receives +a[m] for
 * m = (i - shift) mod 2N < N and -a[m - N] otherwise.  Up to 64 terms go into one launch: a call on words-layout operands
 * issues ceil(n / 64) kernel launches, later groups reading `out` as their addend.  PACKED24 operands are unpacked first.
 * Enqueued on the context's stream, the host does not block; no temporaries are allocated.
 * n = 0 with an addend copies the addend (residues and tag); n = 0 without an addend gives zeros and leaves `out`'s tag as
 * it was.  0 rows or 0 columns succeed with nothing launched.
 * Refused, with nothing launched and `out` (contents AND tag) untouched, every condition checked for every j before the
 * first launch: a null `out`; a null `mats` or `shifts` with n > 0; a null mats[j]; a context, level or shape mismatch of
 * `addend` or any mats[j] with `out`; mixed formats among mats and addend; `out` overlapping any mats[j] (row views share
 * their parent's storage: gpupoly_matrix_row_view); an `addend` that overlaps `out` without being the very same block; a
 * matrix of more than 2^31 (polynomial, 64-slot block) pairs.                                                          */
int gpupoly_matrix_monomial_sum(GpuMatrix *out, const GpuMatrix *addend, const GpuMatrix *const *mats,
                                const uint64_t *shifts, size_t n, int negate);
/* Fused multiply-accumulate (extension):
 *   out[:, dst_col .. dst_col + cols) = addend[:, dst_col .. dst_col + cols) + sgn * sum_{t<n} lhss[t] * rhss[t],
 *   sgn = negate ? -1 : +1.
 * The reference's callers almost never use a product by itself, they add it into something: one output chunk of
 * src/lookup/ggh15/encoding.rs:205-298 is c_b0 M + c_b0 gy_mid + c_b0 v_mid + c_b0 vx_mid - c_b0 pre + sum_inner (input
 * U_inner) v_rhs, written as five add_in_place(&(a * &b)) / x - (a * &b) steps (:224, :244, :255, :273) and an accumulation
 * loop (:275-298); src/lookup/ggh15/pubkey_gpu.rs:408 (target_chunk.add_in_place(&(w_block_v * &v_idx_chunk))) and :494-505;
 * src/lookup/lwe/encoding_gpu.rs:142-223 (two product families per column chunk, summed with add_in_place);
 * src/sampler/trapdoor/gpu.rs:212 (g - (a_bar r + e)) and :286 (public_left p1 + public_right p2);
 * src/gadgets/fhe/ring_gsw_montgomery_gpu.rs:80 (public_matrix randomizer + gadget plaintext); the per-chunk results are
 * then glued with concat_columns_owned (src/slot_transfer/bgg_poly_encoding_gpu.rs:320-335,
 * src/input_injector/diamond_gpu.rs:104-118).  Through gpu_matrix_mul each term is a product launch, an add or sub launch
 * (three more passes over the output), a temporary, a neg launch for a negated term and a copy_block per chunk.
 *   lhss[t]   r x k_t, EVAL;  rhss[t]  k_t x cols, EVAL.  k_t may differ from term to term and may be 0 (adds nothing)
 *   out       r x C with dst_col + cols <= C; columns outside the block are not touched.  Tagged EVAL on success; when the
 *             block is not the whole of `out`, `out` must already be tagged EVAL
 *   addend    NULL, or r x C, EVAL; only its block is read.  With addend == NULL and negate the result is -sum
 * One context and one level (it may be below the context's top level).  The residues are, bit for bit, those of the
 * existing sequence - gpu_matrix_mul per term, gpu_matrix_add / gpu_matrix_sub (or gpupoly_matrix_neg), gpu_matrix_copy_block
 * into place: everything is modular arithmetic on canonical residues, the order of accumulation cannot show.
 * Up to 8 rows: one term-table kernel walks up to 64 terms per launch with lazy accumulators that carry across term
 * boundaries, and its epilogue negates, adds the addend block and stores at dst_col - a call on words-layout operands
 * issues ceil(n / 64) launches (one for n = 0 unless nothing is to be done), later launches reading out's block as their
 * addend.  Above 8 rows every term runs gpu_matrix_mul's tuned kernels into one scratch matrix of the context's allocator
 * (released stream-ordered) followed by one combine pass into the block.  PACKED24 operands are unpacked first.  Enqueued
 * on the context's stream; the host does not block.
 * Overlap: `addend` may be the same block as `out` (accumulate in place: every word is read and written by the same
 * thread), any other overlap of `addend` with `out` is refused; `out` must not overlap any lhss[t] or rhss[t], row views
 * included; operands may repeat and may overlap each other.
 * n = 0 with an addend copies the addend's block into out's block, n = 0 without one writes zeros there; r = 0 or
 * cols = 0 succeed with nothing launched.
 * Refused, with nothing launched and `out` (residues AND tag) untouched, every condition checked for every t before the
 * first launch: a null `out`; null lhss / rhss with n > 0; a null lhss[t] / rhss[t]; a context or level mismatch;
 * lhss[t]->cols != rhss[t]->rows, lhss[t]->rows != out->rows or rhss[t]->cols != cols; dst_col + cols > out->cols; an
 * addend whose shape is not out's; an operand or addend not in EVAL form; a partial block into an `out` not tagged EVAL; the
 * overlaps above (the message contains "overlaps").                                                                   */
int gpupoly_matrix_mul_sum(GpuMatrix *out, size_t dst_col, size_t cols, const GpuMatrix *addend,
                           const GpuMatrix *const *lhss, const GpuMatrix *const *rhss, size_t n, int negate);
/* out += lhs * rhs (negate: out -= lhs * rhs): gpupoly_matrix_mul_sum(out, 0, out->cols, out, &lhs, &rhs, 1, negate), its
 * semantics and refusals (a null matrix is refused; `out` is the addend and must be in EVAL form).                     */
int gpupoly_matrix_mul_acc(GpuMatrix *out, const GpuMatrix *lhs, const GpuMatrix *rhs, int negate);
/* Products with the gadget matrix without the matrix (extension).  G_d = I_d (x) g is d x d*k with
 * dpt = ceil(crt_bits / base_bits), k = small ? dpt : dpt * (level + 1); its column gc = j*k + t*dpt + e (small: j*dpt + e)
 * holds, in row j alone, the constant whose residue in limb l is (2^base_bits mod q_l)^e mod q_l when small || t == l and 0
 * otherwise - exactly what gpu_matrix_fill_gadget / gpu_matrix_fill_small_gadget write.  Of its d * d*k polynomials of L*N
 * words only d*k limb vectors of N words are non-zero, and every BGG+ relation of the reference's callers multiplies by it:
 *   A - G x, A_chunk - G[:, chunk] y, -G[:, chunk], G x: src/lookup/lwe/pubkey_gpu.rs:205-210, src/lookup/lwe/pubkey.rs:449-471,520,
 *     src/lookup/ggh15/pubkey_gpu.rs:393-395,474, src/io/diamond_io/utils.rs:612-616,1664, src/io/diamond_io.rs:684,702,1133,1704,1909,
 *     src/we/diamond_we.rs:223-227, src/lookup/commit_eval.rs:510, src/lookup/debug.rs:290-291,500,
 *     src/gadgets/fhe/ring_gsw_montgomery_gpu.rs:80, src/sampler/trapdoor/gpu.rs:212 (G - (A R + E)),
 *     src/slot_transfer/bgg_poly_encoding.rs:874,1021,1166;
 *   s G and s (G y): src/bgg/sampler_gpu.rs:149, src/bgg/sampler.rs:165,322,524, src/lookup/ggh15/mod.rs:438,
 *     src/lookup/lwe/naive_vec.rs:340, src/slot_transfer/bgg_pubkey.rs:1904, src/slot_transfer/bgg_pubkey_gpu.rs:1607;
 *   G D: src/lookup/ggh15/pubkey_gpu.rs:505 with :1264, src/commit/wee25.rs:718, src/matrix/gpu_dcrt_poly.rs:2114,2159,2406-2479,
 *     src/sampler/trapdoor/sampler.rs:302,315;
 *   a column chunk of G itself: gadget_matrix.slice(0, d, col_start, col_end).
 * Through the existing entries each of these fills the whole of G, runs gpu_matrix_mul_scalar or gpu_matrix_mul over it, then
 * gpu_matrix_add / _sub / gpupoly_matrix_neg and a gpu_matrix_copy_block: d*L times the bytes and, for s G, d times the ring
 * multiplications.
 *
 * gpupoly_matrix_mul_gadget:
 *   out[:, dst_col .. dst_col + cols) = addend[:, dst_col .. dst_col + cols) + sgn * (lhs * G_d[:, gadget_col .. gadget_col + cols)) o scalar,
 *   sgn = negate ? -1 : +1.
 *   lhs         r x d, EVAL; NULL: the identity I_d with d = out->rows
 *   scalar_1x1  NULL: 1; else 1 x 1, EVAL, multiplies every entry point-wise
 *   addend      NULL: 0; else out's shape, EVAL, only its block is read
 *   out         r x C with dst_col + cols <= C; columns outside the block are not touched.  Tagged EVAL on success; when the
 *               block is not the whole of `out`, `out` must already be tagged EVAL
 * Word by word, for entry (i, c), limb l, slot s, with gadget_col + c = (j, t, e): addend +- lhs[i, j][l][s] * w(l, t, e) *
 * scalar[l][s] mod q_l where small || t == l, addend +- 0 elsewhere.  With everything defaulted and cols = d*k the result is
 * gpu_matrix_fill_gadget's, bit for bit; any window of it is the corresponding slice.
 * When `addend` is the same block as `out` (A -= G x) the launch visits only the limb vectors G makes non-zero - r*cols of
 * them (cols with lhs NULL; times L with `small`) - and the others are neither read nor written.  Otherwise one pass writes
 * every limb vector of the block once: a hit reads its lhs vector and the scalar's and addend's, a miss copies the addend's
 * vector or writes zeros.
 *
 * gpupoly_matrix_gadget_mul:  out = addend + sgn * G_d * rhs.
 *   rhs     (d*k) x c, COEFF or EVAL (a constant scales whole limb vectors, so the domain does not matter)
 *   addend  NULL, or d x c in rhs's format
 *   out     d x c, tagged with rhs's format on success
 * Limb l of entry (j, c) is sum_{e<dpt} w(l, l, e) * rhs[j*k + l*dpt + e, c][l] (small: row j*dpt + e): it reads limb l of dpt
 * rows and nothing else - d*k*c*N words of rhs against d*k*c*L*N for the generic product - by Horner with the Shoup constant
 * of 2^base_bits mod q_l.
 *
 * Both: one context and one level (it may be below the context's top level; k follows the level).  The residues are
 * canonical and equal, bit for bit, to those of the existing sequence named above.  Enqueued on the context's stream, the
 * host does not block; no temporaries are allocated (the first call for a base_bits builds a table of dpt weights per limb
 * that the context keeps).  A call on words-layout operands issues exactly one kernel launch; PACKED24 operands are unpacked
 * first.  r = 0, cols = 0, d = 0 or c = 0 succeed with nothing launched.
 * Overlap: `addend` may be the same block as `out` (every word is read and written by the same thread), any other overlap
 * of `addend` with `out` is refused; `out` must not overlap lhs, scalar_1x1 or rhs, row views included (the message contains
 * "overlaps").
 * Refused, with nothing launched and `out` (residues AND tag) untouched, everything checked before the launch, the message
 * naming the entry: a null `out`, a null `rhs`; base_bits of 0 or >= 63; a context or level mismatch; lhs->rows != out->rows;
 * dst_col + cols > out->cols; gadget_col + cols > d*k; rhs->rows != out->rows * k or rhs->cols != out->cols; an addend whose
 * shape is not out's; an lhs, scalar or (mul_gadget) addend not in EVAL form; a scalar that is not 1 x 1; rhs and addend of
 * different formats; a partial block into an `out` not tagged EVAL; the overlaps above.                                   */
int gpupoly_matrix_mul_gadget(GpuMatrix *out, size_t dst_col, const GpuMatrix *lhs, const GpuMatrix *scalar_1x1,
                              size_t gadget_col, size_t cols, const GpuMatrix *addend, int negate, uint32_t base_bits,
                              int small);
/* out = addend + sgn * G_d * rhs: the recomposition half of the pair above - its description, overlap rule (an addend that
 * is `out` is allowed, any other overlap of `out` with addend or rhs is refused) and what is Refused are stated there.  The
 * reference's callers: src/lookup/ggh15/pubkey_gpu.rs:505 with :1264, src/commit/wee25.rs:718 and the relation
 * G * decompose(M) == M of src/matrix/gpu_dcrt_poly.rs:2114,2159; s G of src/bgg/sampler_gpu.rs:149 and A - G x of
 * src/lookup/lwe/pubkey_gpu.rs:205-210 are gpupoly_matrix_mul_gadget's.                                              */
int gpupoly_matrix_gadget_mul(GpuMatrix *out, const GpuMatrix *rhs, const GpuMatrix *addend, int negate,
                              uint32_t base_bits, int small);
/* Extension: the LargeScalarMul gate, lhs * G^-1(G_d o c), without G or its digit matrix.
 *   outs[j] = addends[j] + sgn * lhss[j] * G^-1(G_dj o c),  j < n,  sgn = negate ? -1 : +1.
 * The reference's Evaluables write it as `lhs.mul_decompose(&(M::gadget_matrix(params, d) * scalar))`:
 * src/bgg/public_key.rs:134-140, src/bgg/encoding.rs:191-200 (vector and key matrix), src/bgg/poly_encoding.rs:431-461 (once
 * per slot plus the key), src/bgg/naive_vec.rs:441,607 - gate LargeScalarMul of src/circuit/poly_circuit/eval.rs:343-350.
 * Through the existing entries that is gpu_matrix_fill_gadget, gpu_matrix_mul_scalar and gpupoly_matrix_mul_decompose: a
 * d x dk matrix, a dk x dk digit matrix and a generic product.  Digits are taken per tower and entry (j, (j, t, e)) of G o c is
 * non-zero in limb t only, so G^-1(G_d o c) = I_d (x) blockdiag_t(D_t) with D_t[e'][e] the polynomial whose coefficient i is
 * digit e' of (c_t[i] * B^e mod q_t), B = 2^base_bits, written into every limb and transformed, and
 *   out[i, (j, t, e)] = sum_{e' < dpt} lhs[i, (j, t, e')] * D_t[e'][e]      (every limb, every slot):
 * L*dpt^2 digit polynomials instead of (d*k)^2, dpt ring multiplications per output instead of d*k.
 *   k = dpt * (level + 1), dpt = ceil(crt_bits / base_bits)
 *   lhss[j]     rows_j x (d_j * k), EVAL; rows_j and d_j may differ between operands and may be 0
 *   outs[j]     lhss[j]'s shape, made by the caller, tagged EVAL on success
 *   addends     NULL, or addends[j] NULL: no addend; else outs[j]'s shape, EVAL
 *   scalar_1x1  1 x 1, COEFF or EVAL, left untouched (an EVAL scalar is inverse-transformed into scratch)
 *   const_words host memory: words_per_const >= 1 little-endian 64-bit words of an integer C of any size, reduced mod every
 *               q_t in the entry (gpupoly_matrix_load_coeff_words's rule; from_biguints(&[C]) of the reference)
 * One context and one level per call (it may be below the top; scalar_1x1 is at that level).  The residues are canonical and
 * equal, bit for bit, to those of gpu_matrix_fill_gadget, gpu_matrix_mul_scalar, gpupoly_matrix_mul_decompose and
 * gpu_matrix_add / _sub / gpupoly_matrix_neg.  Enqueued on the context's stream, the host does not block; temporaries come
 * from the context's allocator and are released stream-ordered; PACKED24 operands are unpacked first; n = 0 does nothing.
 * _const_many: every D_t[e'][e] is a constant below 2^base_bits, its own transform - L^2*dpt^2 weights built on the host, no
 * transform at all, ceil(n' / 64) launches for the n' operands that have entries, lhs read once and out written once.  The
 * context keeps the weights per constant, as it keeps the gadget weight table: the first call for a constant uploads them
 * (synchronous, once), later calls only launch.
 * _scalar_many: one table kernel and one forward transform over L*dpt^2 polynomials per call, then one product launch per 64
 * operands.  When the table (L^2*dpt^2*N words) exceeds gpupoly_matrix_mul_decompose's budget rule it is built and used in
 * groups of towers; MXX_HIP_GADGET_SCALAR_BUDGET=<bytes> overrides the budget for this entry.
 * Overlap: addends[j] may be the same block as outs[j] (every word is read and written by the same thread); outs[j] must not
 * overlap any lhs, the scalar, another output or another operand's addend, row views included; any other overlap of an addend
 * with an output is refused (the message contains "overlaps").
 * Refused, with nothing launched and every outs[j] (residues AND tag) untouched, everything checked for every j before the
 * first launch, the message naming the entry: null outs or lhss with n > 0; a null outs[j] or lhss[j]; a null scalar_1x1; a
 * null const_words or words_per_const = 0; base_bits of 0 or >= 63; a context or level mismatch; lhss[j]->cols not a multiple
 * of k; an out or addend whose shape is not the lhs's; an lhs or addend not in EVAL form; a scalar that is not 1 x 1; the
 * overlaps above.                                                                                                        */
int gpupoly_matrix_mul_decompose_gadget_scalar_many(GpuMatrix *const *outs, const GpuMatrix *const *lhss,
                                                    const GpuMatrix *const *addends, size_t n, const GpuMatrix *scalar_1x1,
                                                    int negate, uint32_t base_bits);
/* The same gate for an integer constant C (const_words): its description, overlap rule and what is Refused are stated above -
 * any overlap of outs[j] with an lhs, another output or another operand's addend is refused, an addend that is outs[j]'s own
 * block is allowed.  The reference's callers pass &[shift], &[p_full], &[reconst_coeff]: src/bgg/public_key.rs:134-140,
 * src/bgg/encoding.rs:191-200, src/bgg/poly_encoding.rs:431-461.                                                          */
int gpupoly_matrix_mul_decompose_gadget_const_many(GpuMatrix *const *outs, const GpuMatrix *const *lhss,
                                                   const GpuMatrix *const *addends, size_t n, const uint64_t *const_words,
                                                   size_t words_per_const, int negate, uint32_t base_bits);
/* kernel launches issued by the library since it was loaded (every context; copies / memsets not counted): bench.py
 * reports launches per step for the launch-bound small-ring chain                                              */
uint64_t gpupoly_launch_count(void);
/* Test instrument: evaluates the samplers' deterministic math (mxx_amd/csrc/detmath.h) ON THE DEVICE for n host-supplied
 * doubles - fn 0: log(x), 1: cos(2 pi x), 2: sqrt(-2 log x) - and copies the results back (synchronous).  The Box-Muller
 * step of the G-lattice sampler (cuda/src/matrix/MatrixTrapdoor.cu:701-833 calls log / cos there) is the only place on the
 * path with transcendental functions; this lets a test hold the device's results to libm (log and sqrt(-2 log) within 2 ulp, cos(2 pi x) within 3). */
int gpupoly_detmath_eval(GpuContext *ctx, int fn, const double *host_in, double *host_out, size_t n);
/* 1 if `device` can address `peer`'s memory directly (xGMI peer mapping; a device always reaches itself) */
int gpupoly_device_can_access_peer(int device, int peer, int *out_can);
/* a one-thread no-op kernel (`gpupoly_marker_kernel`) on the context's stream: delimits bench.py's timed region in a
 * profiler's dispatch list (tools/pmc_window.py counts only what lies between two markers)                     */
int gpupoly_marker_launch(GpuContext *ctx, uint32_t id);
/* Launch trace (bench.py's composed roofline of a multi-kernel call: a preimage, a chain step).  Between _begin and
 * _end every kernel launch and every device-to-device copy of the library - any context, any host thread - is
 * bracketed by two hipEvents on the stream it is enqueued on.  _end stops recording, waits for the recorded work and
 * returns one line per launch in launch order: "kernel \t blocks \t threads \t algorithmic bytes \t ms \n" (bytes = the
 * launch's operands read once + written once, 0 where the launcher does not state them).  The string belongs to the
 * library and stays valid until the next _begin / _end; NULL on error.  Tracing costs two event records per launch:
 * durations are the kernels' own, the call's wall time is not what an untraced call takes.                       */
int gpupoly_trace_begin(void);
const char *gpupoly_trace_end(void);
const char *gpupoly_version(void);
/* MXX_HIP_* switches are read once, at gpu_context_create; this re-reads them for every live
 * context of the process (tests flip them between calls).                      */
int gpupoly_reload_env(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUPOLY_H */
