"""The nested-RNS encoding helpers of the reference (src/gadgets/arith/nested_rns/encoding.rs) over the device entries
of DESIGN.md section 5z: the gadget vector, the gadget decomposition and the p-residues of a matrix are one call each
(gpupoly_matrix_fill_nested_rns_gadget, gpupoly_matrix_nested_rns_decompose, gpupoly_matrix_nested_rns_residues)
instead of the reference's host loop over BigUints per coefficient (map_nested_rns_values, encoding.rs:121-139)."""
from math import gcd

from .matrix import GpuDCRTPolyMatrix


def mul_budget_bound(sum_p_moduli: int, modulus_count: int, q_max: int) -> int:
    """`sample_crt_primes_mul_budget_bound` (encoding.rs:14-22)."""
    return (sum_p_moduli + modulus_count) * q_max // 2


def sample_crt_primes(max_bit_width: int, q_max: int, max_unreduced_muls: int) -> list:
    """`sample_crt_primes` (encoding.rs:39-71): the first pairwise coprime integers from 3 up, below 2^max_bit_width,
    until their product exceeds bound^max_unreduced_muls.  Deterministic; not all prime (3, 4, 5, 7, 11, ...)."""
    chosen, total, prod = [], 0, 1
    for candidate in range(3, 1 << max_bit_width):
        if all(gcd(candidate, c) == 1 for c in chosen):
            chosen.append(candidate)
            total += candidate
            prod *= candidate
        if mul_budget_bound(total, len(chosen), q_max) ** max_unreduced_muls < prod:
            return chosen
    raise ValueError(f"failed to find enough pairwise coprime integers with bit width {max_bit_width} to satisfy "
                     f"q_max {q_max} and max_unreduced_muls {max_unreduced_muls}")


class NestedRnsContext:
    """The integers of `NestedRnsPolyContext::setup` that the encoding helpers read: the q moduli of `params` (the first
    q_level of them), the p moduli `sample_crt_primes` picks for them, and the scale of the rounded sum."""

    def __init__(self, params, p_moduli_bits: int, max_unreduced_muls: int, scale: int, q_level=None):
        q_moduli, _, depth = params.to_crt()
        self.params = params
        self.q_moduli = [int(q) for q in q_moduli]
        self.q_moduli_depth = depth if q_level is None else q_level
        assert 1 <= self.q_moduli_depth <= depth, "q_level exceeds the CRT depth"
        self.p_moduli = sample_crt_primes(p_moduli_bits, max(self.q_moduli), max_unreduced_muls)
        self.max_unreduced_muls = max_unreduced_muls
        self.scale = int(scale)

    def chunk_width(self) -> int:
        return len(self.p_moduli) + 1

    def active_window(self, enable_levels=None, level_offset=None):
        """`resolve_nested_rns_active_window` (encoding.rs:146-160): (level_offset, active_levels)."""
        off = 0 if level_offset is None else level_offset
        assert off <= self.q_moduli_depth, "level_offset must not exceed q_moduli_depth"
        levels = self.q_moduli_depth - off if enable_levels is None else enable_levels
        assert off + levels <= self.q_moduli_depth, "active range exceeds q_moduli_depth"
        return off, levels

    def gadget_vector(self, enable_levels=None, level_offset=None, eval_format: bool = True) -> GpuDCRTPolyMatrix:
        """`nested_rns_gadget_vector` (encoding.rs:240-271)."""
        off, levels = self.active_window(enable_levels, level_offset)
        return GpuDCRTPolyMatrix.nested_rns_gadget_vector(self.params, self.p_moduli, self.scale, off, levels, eval_format)

    def gadget_decomposed(self, value: GpuDCRTPolyMatrix, enable_levels=None, level_offset=None,
                          eval_format: bool = True) -> GpuDCRTPolyMatrix:
        """`nested_rns_gadget_decomposed` (encoding.rs:273-338)."""
        off, levels = self.active_window(enable_levels, level_offset)
        return value.nested_rns_decompose(self.p_moduli, self.scale, off, levels, eval_format)

    def residues(self, value: GpuDCRTPolyMatrix, enable_levels=None, level_offset=None) -> GpuDCRTPolyMatrix:
        """Coefficient by coefficient what `encode_nested_rns_poly_with_offset` gives for one integer: rows
        (row * levels + a) * D + j hold (residue in limb off + a) mod p_j."""
        off, levels = self.active_window(enable_levels, level_offset)
        return value.nested_rns_residues(self.p_moduli, off, levels)

    def encode_poly(self, value: int, enable_levels=None, level_offset=None) -> list:
        """`encode_nested_rns_poly_with_offset` (encoding.rs:401-420): the constant polynomials (value mod q_a) mod p_j,
        q-level major."""
        from .poly import GpuDCRTPoly

        off, levels = self.active_window(enable_levels, level_offset)
        return [GpuDCRTPoly.from_biguint_to_constant(self.params, (int(value) % q) % p)
                for q in self.q_moduli[off:off + levels] for p in self.p_moduli]
