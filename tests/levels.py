"""Matrices below the top level: the contexts, helpers and the coverage table of tests/test_gpu_levels.py.

The level rule.  A matrix at level l of a context of D limbs uses the PREFIX q_0 .. q_l of the basis: its words are
[poly][l + 1][N], limb i of the matrix is limb i of the context, and every per-limb table of the context (twiddles,
LimbConst, Garner, weights) is indexed by that i.  What does not shrink with the level is what the context decided once
from ALL D moduli: the word width, lazy_ok / tight_ok / f64_ok / pack24_ok, and crt_bits - so the digits per tower,
dpt = ceil(crt_bits(all D moduli) / base_bits), come from the context and k = dpt * (l + 1) from both.  A launcher that
confuses the two limb counts is right at l = D - 1 and wrong below it.

The references are the plain ones handed the truncated basis moduli[: l + 1] (oracle.matrix_ntt, oracle.matmul,
oracle.pointwise, the oracle's samplers; plainref.digits with the context's dpt stated explicitly).

TABLE maps every C-ABI entry of include/gpupoly.h that takes a GpuMatrix to what proves it below the top level;
tests/test_level_table_host.py checks the table against the header and the test modules without a GPU.
"""
import re

import numpy as np

import plainref

# name -> ("gen", depth, bits): oracle.gen_crt_basis(n, depth, bits); ("bits", (b0, b1, ...)): the largest primes = 1 (mod 2n)
# of those widths, limb by limb (the matrix's own limbs belong to another class than the context's)
CONTEXTS = {
    "24": ("gen", 4, 24),         # 32-bit words: lazy + signed + pack24
    "28": ("gen", 3, 28),         # 32-bit words: TIGHT
    "31": ("gen", 3, 31),         # 32-bit words: neither lazy nor tight
    "51": ("gen", 3, 51),         # 64-bit words: double precision
    "58": ("gen", 3, 58),         # 64-bit words: integer
    "24_24_31": ("bits", (24, 24, 31)),  # 32-bit words, not lazy_ok; the matrix at level 1 has 24-bit limbs only
    "28_28_51": ("bits", (28, 28, 51)),  # 64-bit words; the matrix at level 1 has narrow limbs only
}
BASE_BITS = {"24": 12, "28": 14, "31": 8, "51": 17, "58": 20, "24_24_31": 8, "28_28_51": 17}
GEN = ("24", "28", "31", "51", "58")
MIXED = ("24_24_31", "28_28_51")
MFMA_MAX_Q = 16711424  # mmfma::MAX_Q (matmul_mfma.hip), as in tests/test_gpu_surface.py


def depth_of(ctx):
    kind, *rest = CONTEXTS[ctx]
    return rest[0] if kind == "gen" else len(rest[0])


def levels_of(ctx):
    """level 0 and level D - 2 (the top level is the existing suite); the mixed-width contexts run at level 1 only"""
    if ctx in MIXED:
        return (1,)
    return tuple(sorted({0, depth_of(ctx) - 2}))


def basis(oracle, ctx, n):
    kind, *rest = CONTEXTS[ctx]
    if kind == "gen":
        return [int(q) for q in oracle.gen_crt_basis(n, rest[0], rest[1])]
    out = []
    for bits in rest[0]:
        out.append(next(q for q in plainref.primes(n, bits, len(rest[0])) if q not in out))
    return out


def mfma_basis(n, count=3):
    """the "below MAX_Q" rule of tests/test_gpu_surface.py with one more limb: the largest primes = 1 (mod 2n) that the
    matrix-core kernel still takes"""
    out, q = [], MFMA_MAX_Q - 1 - (MFMA_MAX_Q - 2) % (2 * n)
    while len(out) < count:
        if plainref.is_prime(q):
            out.append(q)
        q -= 2 * n
    return out


_PARAMS = {}


def params(gpu, oracle, ctx, n, base_bits=None, prefix=None):
    """the context `ctx` at ring n; prefix = l: the SECOND context over moduli[: l + 1] (same n, base_bits and width class)"""
    base_bits = BASE_BITS[ctx] if base_bits is None else base_bits
    key = (ctx, n, base_bits, prefix)
    if key not in _PARAMS:
        moduli = basis(oracle, ctx, n)
        _PARAMS[key] = gpu.GpuDCRTPolyParams(n, moduli if prefix is None else moduli[: prefix + 1], base_bits)
    return _PARAMS[key]


def dpt_of(p):
    """digits per tower: always from the context's D moduli"""
    return -(-p.crt_bits() // p.base_bits())


def host(oracle, seed, rows, cols, moduli, n, edges=True):
    """(rows, cols, L, n) residues of the truncated basis: random, with polynomial 0 all q_l - 1 and polynomial 1 zero where
    there are that many (one polynomial: its first coefficients q_l - 1, its last ones zero)"""
    x = oracle.random_matrix(seed, rows, cols, moduli, n)
    if not edges:
        return x
    top = (np.asarray(moduli, dtype=np.uint64) - np.uint64(1)).reshape(-1, 1)
    flat = x.reshape(rows * cols, len(moduli), n)
    if rows * cols >= 3:
        flat[0] = top
        flat[1] = 0
    elif rows * cols:
        flat[0, :, : max(n // 8, 1)] = top
        flat[0, :, n - max(n // 8, 1):] = 0
    return x


def ref_digits(x, moduli, base_bits, dpt, small=False):
    """G^-1 of the (rows, cols, L, n) coefficient array at the truncated basis with the context's dpt: (rows * k, cols, L, n),
    row j * k + t * dpt + e = digit e of tower t of x[j, .] (small: the digits of tower 0 only, k = dpt)"""
    rows, cols, L, n = x.shape
    k = dpt if small else dpt * L
    out = np.zeros((rows * k, cols, L, n), dtype=np.uint64)
    for j in range(rows):
        for c in range(cols):
            out[j * k:(j + 1) * k, c] = plainref.digits(x[j, c], moduli, base_bits, dpt)[:k]
    return out


def ref_gadget(size, moduli, base_bits, dpt, n, small=False):
    """I_size (x) g at the truncated basis with the context's dpt, coefficient form (plainref.gadget derives dpt from the
    moduli it is given, which is the context's only in same-width bases)"""
    L = len(moduli)
    k = dpt if small else dpt * L
    out = np.zeros((size, size * k, L, n), dtype=np.uint64)
    for r in range(size):
        for t in range(1 if small else L):
            for e in range(dpt):
                for l in range(L):
                    if small or l == t:
                        out[r, r * k + t * dpt + e, l, 0] = pow(2, e * base_bits, int(moduli[l]))
    return out


def new(gpu, p, rows, cols, level, is_ntt):
    return gpu.GpuDCRTPolyMatrix(p, rows, cols, level, is_ntt)


def call(entry, *args):
    from mxx_amd import _ffi

    _ffi.check_status(getattr(_ffi.lib(), entry)(*args), entry)


def arr(ms):
    import ctypes as C

    return (C.c_void_p * max(len(ms), 1))(*[m.raw.value if hasattr(m.raw, "value") else m.raw for m in ms])


def seed_bytes(tag):
    return bytes((tag * 41 + 13 * i + 7) & 0xFF for i in range(32))


def prototypes(header_text):
    """{entry: argument text} of every prototype of the header that takes a GpuMatrix"""
    s = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    s = re.sub(r"^\s*#.*$", "", s, flags=re.M)
    out = {}
    for m in re.finditer(r"\b(?:int|void|const char \*)\s*\*?\s*(\w+)\s*\(([^;{}]*?)\)\s*;", s, flags=re.S):
        args = " ".join(m.group(2).split())
        if "GpuMatrix" in args:
            out[m.group(1)] = args
    return out


def writes_a_matrix(args):
    """whether the prototype takes a matrix it may write: a GpuMatrix pointer that is not const"""
    return re.search(r"(?<!const )GpuMatrix \*", args) is not None


# ---- the coverage table -------------------------------------------------------------------------------------------------------
# entry -> a tuple of "module::test" ids that run it on matrices below the top level (its own kernels at L < limb_count), or
#          ("refuses", "module::test"): the entry turns such a matrix away and that test asserts it, or
#          ("no limbs", reason): its work does not depend on the level.
_L = "test_gpu_levels::"
_TRANSFORMS = (_L + "test_transforms_forward_inverse_and_tag",)
_STRUCTURE = (_L + "test_pointwise_and_structure",)
_PRODUCTS = (_L + "test_product_families", _L + "test_product_register_tiles", _L + "test_product_matrix_cores",
             _L + "test_product_default_dispatch_and_batch")
_DECOMPOSE = (_L + "test_decompose_and_gadgets",)
_DECOMPOSED = (_L + "test_decomposed_products_and_identity_chunk",)
_PREIMAGE = (_L + "test_preimage_many_and_keyed",)
_ODDS = (_L + "test_views_pointers_wire_aliases_hashed_blocks_and_mul_acc",)
_LOW = "test_operands_below_the_top_level_equal_the_plain_reference"

TABLE = {
    "gpu_matrix_create": _STRUCTURE,
    "gpu_matrix_destroy": ("no limbs", "returns the storage to the context's allocator whatever its size; nothing is computed"),
    "gpu_matrix_copy": _STRUCTURE,  # clone()
    "gpu_matrix_copy_block": _STRUCTURE,
    "gpu_matrix_add": _STRUCTURE,
    "gpu_matrix_sub": _STRUCTURE,
    "gpu_matrix_add_block": _STRUCTURE,
    "gpu_matrix_mul": _PRODUCTS,
    "gpu_matrix_mul_scalar": _STRUCTURE,
    "gpu_matrix_equal": _STRUCTURE + (_L + "test_equal_answers_not_equal_across_levels_without_an_error", "test_gpu_equal_verdict::test_extent_of_views_and_levels"),
    "gpu_matrix_ntt_all": _TRANSFORMS,
    "gpu_matrix_intt_all": _TRANSFORMS,
    "gpu_matrix_fill_gadget": _DECOMPOSE,
    "gpu_matrix_fill_small_gadget": _DECOMPOSE,
    "gpu_matrix_fill_small_decomposed_identity_chunk": _DECOMPOSED,
    "gpu_matrix_decompose_base": _DECOMPOSE,
    "gpu_matrix_decompose_base_small": _DECOMPOSE,
    "gpu_matrix_sample_distribution": (_L + "test_plain_samplers", _L + "test_uniform_sample_at_2_14_is_packed_below_the_top"),
    "gpu_matrix_sample_distribution_columns": (_L + "test_plain_samplers",),
    "gpu_matrix_gauss_samp_gq_arb_base": (_L + "test_gauss_samp_gq",),
    "gpu_matrix_sample_p1_full": (_L + "test_p1_sampler_full_and_cached",),
    "gpu_matrix_create_p1_covariance_cache": (_L + "test_p1_sampler_full_and_cached",) + _PREIMAGE,
    "gpu_matrix_sample_p1_full_cached": (_L + "test_p1_sampler_full_and_cached",),
    "gpu_matrix_load_rns_batch": (_L + "test_movement",),
    "gpu_matrix_store_rns_batch": (_L + "test_movement",),
    "gpu_matrix_store_const_coeff_batch": (_L + "test_movement",),
    "gpu_matrix_store_compact_bytes": _ODDS + ("test_gpu_serde::test_compact_bytes_lower_level_and_large",),
    "gpu_matrix_load_compact_bytes": _ODDS + ("test_gpu_serde::test_compact_bytes_lower_level_and_large",),
    "gpu_poly_store_compact_bytes": _ODDS,
    "gpu_poly_load_compact_bytes": _ODDS,
    "gpupoly_matrix_mul_decompose": _DECOMPOSED,
    "gpupoly_matrix_mul_decompose_many": ("test_gpu_mul_decompose_many::test_a_level_below_the_top",),
    "gpupoly_matrix_mul_decompose_pairs": ("test_gpu_mul_decompose_pairs::test_a_level_below_the_top",),
    "gpupoly_matrix_mul_batch": (_L + "test_product_default_dispatch_and_batch",),
    "gpupoly_matrix_mul_decompose_small": _DECOMPOSED,
    "gpupoly_matrix_mul_tensor_identity": _DECOMPOSED,
    "gpupoly_matrix_mul_tensor_identity_decompose": _DECOMPOSED,
    "gpupoly_matrix_mul_scalar_intt": (_L + "test_fused_transform_variants",),
    "gpupoly_matrix_transpose": _STRUCTURE,
    "gpupoly_matrix_tensor": _STRUCTURE,
    "gpupoly_matrix_add_rows": (_L + "test_fused_transform_variants",),
    "gpupoly_matrix_ntt_add_rows": (_L + "test_fused_transform_variants",),
    "gpupoly_matrix_row_view": _ODDS,
    "gpupoly_matrix_reshape_view": _ODDS,
    "gpupoly_matrix_neg": _STRUCTURE,
    "gpupoly_matrix_fill_zero": _STRUCTURE,
    "gpupoly_matrix_fill_identity": _STRUCTURE,
    "gpupoly_matrix_sample_decomposed": _DECOMPOSED,
    "gpupoly_matrix_decompose_rows": _DECOMPOSE,
    "gpupoly_matrix_sample_decomposed_window": ("test_gpu_decomposed_blocks::test_an_output_below_the_top_level",),
    "gpupoly_matrix_device_ptr": _ODDS,
    "gpupoly_matrix_layout": (_L + "test_uniform_sample_at_2_14_is_packed_below_the_top",),
    "gpupoly_matrix_copy_to_context": (_L + "test_movement",),
    "gpupoly_matrix_all_gather_columns": (_L + "test_movement",),
    # the three segmented samplers are what a batched preimage at the level is made of (preimage_group, preimage.hip)
    "gpupoly_matrix_sample_distribution_segments": _PREIMAGE,
    "gpupoly_matrix_sample_p1_full_cached_segments": _PREIMAGE,
    "gpupoly_matrix_gauss_samp_gq_arb_base_segments": _PREIMAGE,
    "gpupoly_matrix_sample_distribution_blocks": _ODDS + ("test_gpu_sample_blocks::test_an_output_below_the_top_level_through_the_raw_entries",),
    "gpupoly_matrix_sample_hash_blocks": _ODDS,
    "gpupoly_matrix_sample_gauss_blocks": _ODDS + ("test_gpu_gauss_blocks::test_an_output_below_the_top_level_through_the_raw_entries",),
    "gpupoly_matrix_sample_hash_gauss_blocks": _ODDS,
    "gpupoly_matrix_concat_columns": _STRUCTURE,
    "gpupoly_matrix_split_columns": _STRUCTURE,
    "gpupoly_trapdoor_preimage_many": _PREIMAGE,
    "gpupoly_trapdoor_preimage_keyed": _PREIMAGE,
    "gpupoly_matrix_sample_decomposed_blocks": ("test_gpu_decomposed_blocks::test_an_output_below_the_top_level",),
    "gpupoly_matrix_sample_hash_decomposed_blocks": ("test_gpu_decomposed_blocks::test_an_output_below_the_top_level",),
    "gpupoly_matrix_lut_targets": ("test_gpu_lut_targets::" + _LOW,),
    "gpupoly_matrix_lut_targets_combine": ("test_gpu_lut_targets::" + _LOW,),
    "gpupoly_matrix_lwe_targets": ("test_gpu_lwe_targets::" + _LOW,),
    "gpupoly_matrix_lwe_targets_combine": ("test_gpu_lwe_targets::" + _LOW,),
    "gpupoly_matrix_wee25_targets": ("test_gpu_wee25_targets::" + _LOW,),
    "gpupoly_matrix_wee25_targets_product": ("test_gpu_wee25_targets::" + _LOW,),
    "gpupoly_matrix_ggh15_lookup": ("test_gpu_ggh15_lookup::" + _LOW,),
    "gpupoly_matrix_ggh15_lookup_combine": ("test_gpu_ggh15_lookup::" + _LOW,),
    "gpupoly_matrix_lwe_lookup": ("test_gpu_lwe_lookup::" + _LOW,),
    "gpupoly_matrix_lwe_lookup_combine": ("test_gpu_lwe_lookup::" + _LOW,),
    "gpupoly_matrix_slot_transfer_eval": ("test_gpu_slot_transfer_eval::" + _LOW,),
    "gpupoly_matrix_slot_transfer_eval_combine": ("test_gpu_slot_transfer_eval::" + _LOW,),
    # exact scaling needs every limb of the basis: an input or output below full level is "unsupported" / a level mismatch
    "gpupoly_matrix_scale_round": ("refuses", "test_gpu_scale_round::test_unsupported_inputs_fall_back_to_the_host_path"),
    "gpupoly_matrix_crt_recompose_rounded": ("refuses", "test_gpu_crt_recompose::test_refusals_launch_nothing_and_leave_the_output_alone"),
    "gpupoly_matrix_nested_rns_decompose": ("test_gpu_nested_rns::test_table_slice_beyond_lds_and_source_below_full_level",),
    "gpupoly_matrix_fill_nested_rns_gadget": ("test_gpu_nested_rns::test_table_slice_beyond_lds_and_source_below_full_level",),
    "gpupoly_matrix_nested_rns_residues": ("test_gpu_nested_rns::test_table_slice_beyond_lds_and_source_below_full_level",),
    "gpupoly_matrix_store_coeff_words": ("test_gpu_scale_round::test_store_coeff_words_matches_crt_and_refuses_short_words",),
    "gpupoly_matrix_load_coeff_words": ("test_gpu_load_coeff_words::test_one_word_short_polys_and_lower_levels",),
    "gpupoly_matrix_centered_max_abs": ("test_gpu_centered_norm::test_matches_big_integers",),
    "gpupoly_matrix_extract_bits": ("test_gpu_readout::test_extract_bits_matches_python",),
    "gpupoly_matrix_store_coeff_ints": ("test_gpu_readout::test_coeffs_ints_match_python",),
    "gpupoly_matrix_store_compact_bytes_many": ("test_gpu_compact_many::test_mixed_levels_in_one_call",),
    "gpupoly_matrix_load_compact_bytes_many": ("test_gpu_compact_many::test_mixed_levels_in_one_call",),
    "gpupoly_matrix_fill_monomial": ("test_gpu_monomial::test_level_0_of_a_three_limb_context",),
    "gpupoly_matrix_mul_monomial": ("test_gpu_monomial::test_level_0_of_a_three_limb_context",),
    "gpupoly_matrix_monomial_sum": ("test_gpu_monomial::test_level_0_of_a_three_limb_context",),
    "gpupoly_matrix_mul_sum": ("test_gpu_mul_sum::test_a_level_below_the_top",),
    "gpupoly_matrix_mul_acc": _ODDS,
    "gpupoly_matrix_mul_gadget": ("test_gpu_gadget_products::test_mul_gadget_at_a_level_below_the_top",),
    "gpupoly_matrix_gadget_mul": ("test_gpu_gadget_products::test_gadget_mul_at_a_level_below_the_top",),
    "gpupoly_matrix_mul_decompose_gadget_scalar_many": ("test_gpu_gadget_scalar::test_a_level_below_the_top",),
    "gpupoly_matrix_mul_decompose_gadget_const_many": ("test_gpu_gadget_scalar::test_a_level_below_the_top",),
}
