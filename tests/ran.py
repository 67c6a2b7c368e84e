"""Which kernels ran: the launch trace as a context manager, and the table of what every forced switch must launch.

A test that sets an MXX_HIP_* switch and then compares values proves nothing about the switch: every dispatcher falls
back to another correct kernel when the forced one declines, and EnvSwitches::load maps a spelling it does not know to
the default.  Such a test wraps the forced call in `launches()` and asserts, from TABLE, that the family the switch names
ran and that the default family did not.  Products are checked through `params.ctx().last_kernel()` instead (the entries
with `last`).  tests/test_ran_table_host.py checks on the CPU that every (switch, value, word class) below has an
asserting case in every test that uses it.

TABLE was written by reading the dispatchers (launch_ntt_typed in ntt.hip, launch_ntt_lds / launch_ntt14 / DigitLaunch in
ntt_rings.h, launch_ntt_lds_u64 in ntt_lds_u64.hip, launch_mul_intt_u32 in ntt_lds_u32.hip, decompose_segment in
decompose.hip, the compact store in serde.hip, gpupoly_matrix_mul_sum in matmul_sum.hip, launch_matmul in arith.hip), not
by running them.  A launch's name is the stringified kernel expression of its MXX_LAUNCH, template arguments as the
source spells them: `ntt14::inv_kernel<W, true>`, `nttf::fwd_kernel<R::LOGN, R::LOGR, R::WPE, ELIM, NT()>`.

Word classes, by what the dispatchers look at first: "u32" - every modulus below 2^31, 32-bit words; "u64f" - 64-bit
words with every modulus at most 51 bits, where the double-precision transforms (nttf::) are the default; "u64" - 64-bit
words beyond 51 bits.

Where "large" starts for the two grid-stride kernels that most tests lean on (arith.hip): equal_kernel is capped at
8192 blocks of 256 threads, one word per thread and trip, so it strides from 2 097 153 words (8192 * 256 + 1);
elementwise_kernel is capped at 16384 blocks of 256 threads with one 16-byte vector per thread and trip, so it strides
from 16 777 217 words in 32-bit contexts (4 words per vector), from 8 388 609 words in 64-bit contexts (2 per vector),
and from 4 194 305 words in the scalar form of rings shorter than a vector (n < 4, or n < 2 in 64-bit words).
"""
import contextlib
from collections import namedtuple

from mxx_amd import _ffi

# ran / forward / inverse: every item needs a launch whose name starts with it (a tuple: with one of its alternatives);
# `forward` and `inverse` are asked where the block ran a transform in that direction, `ran` always; absent: no launch may
# start with any of these; last: what ctx.last_kernel() must start with after a product
Expect = namedtuple("Expect", "ran forward inverse absent last", defaults=((), (), (), (), None))

_TUNED = ("ntt_fwd_lazy_kernel", "ntt_inv_lazy_kernel", "ntt_fwd_head_kernel", "ntt_inv_tail_kernel", "ntt14::", "nttf::")
_DIGITS = ("ntt14::fwd_digits_kernel", "nttf::fwd_digits_kernel", "nttf::head_kernel<R::PRE, ELIM, true",
           "ntt_fwd_lazy_digits_kernel", "ntt_fwd_head_digits_kernel")
_PLAIN_DIGITS = ("decompose_kernel", "decompose_rows_kernel")
_ALL = ("u32", "u64f", "u64")


def _every(e, classes=_ALL):
    return {c: e for c in classes}


_GROUPED = Expect(forward=("ntt14::fwd_kernel",), inverse=("ntt14::inv_kernel<W, true",),
                  absent=("ntt14::inv_kernel<W, false", "ntt_fwd_lazy_kernel", "ntt_inv_lazy_kernel", "ntt_generic_kernel",
                          "ntt_stage_global_kernel"))
_FUSED_ON = {
    "u32": Expect(ran=(("ntt14::fwd_digits_kernel", "ntt_fwd_lazy_digits_kernel", "ntt_fwd_head_digits_kernel"),), absent=_PLAIN_DIGITS),
    "u64f": Expect(ran=(("nttf::fwd_digits_kernel", "nttf::head_kernel<R::PRE, ELIM, true"),), absent=_PLAIN_DIGITS),
    "u64": Expect(ran=(("ntt_fwd_lazy_digits_kernel", "ntt_fwd_head_digits_kernel"),), absent=_PLAIN_DIGITS + ("nttf::",)),
}
_SERDE_FAST = Expect(ran=(("compact_maxbits_fast_kernel", "compact_maxbits_many_kernel"),))
_REG = Expect(last="matmul_kernel<u32")

# (switch, value) -> {word class: Expect}; value None: the switch unset.  A class that is missing is one the switch does
# not apply to (MXX_HIP_NTT14 and MXX_HIP_MATMUL_* are read for 32-bit words only, MXX_HIP_NTT64 where nttf:: is the default)
TABLE = {
    ("MXX_HIP_NTT_PATH", "generic"): _every(Expect(forward=("ntt_generic_kernel",), inverse=("ntt_generic_kernel",), absent=_TUNED + ("ntt_stage_global_kernel",))),
    ("MXX_HIP_NTT_PATH", "global"): _every(Expect(forward=("ntt_stage_global_kernel",), inverse=("ntt_stage_global_kernel", "ntt_scale_global_kernel"),
                                                  absent=_TUNED + ("ntt_generic_kernel",))),
    # 2^14 points in 32-bit words.  The signed grouped inverse is <W, true...>, the unsigned one <W, false...>
    ("MXX_HIP_NTT14", None): {"u32": _GROUPED},
    ("MXX_HIP_NTT14", "grouped"): {"u32": _GROUPED},
    ("MXX_HIP_NTT14", "unsigned"): {"u32": Expect(forward=("ntt14::fwd_kernel",), inverse=("ntt14::inv_kernel<W, false",),
                                                  absent=("ntt14::inv_kernel<W, true", "ntt_fwd_lazy_kernel", "ntt_inv_lazy_kernel",
                                                          "ntt_generic_kernel", "ntt_stage_global_kernel"))},
    ("MXX_HIP_NTT14", "whole"): {"u32": Expect(forward=("ntt_fwd_lazy_kernel",), inverse=("ntt_inv_lazy_kernel",),
                                               absent=("ntt14::", "ntt_generic_kernel", "ntt_stage_global_kernel"))},
    # every integer transform kernel starts with "ntt_", no double-precision one does
    ("MXX_HIP_NTT64", None): {"u64f": Expect(ran=("nttf::",), absent=("ntt_",))},
    ("MXX_HIP_NTT64", "int"): {"u64f": Expect(ran=("ntt_",), absent=("nttf::",))},
    ("MXX_HIP_DECOMPOSE_FUSED", None): _FUSED_ON,
    ("MXX_HIP_DECOMPOSE_FUSED", "1"): _FUSED_ON,
    ("MXX_HIP_DECOMPOSE_FUSED", "0"): _every(Expect(ran=(_PLAIN_DIGITS,), absent=_DIGITS)),
    # the store of one matrix (compact_*_fast_kernel) and of many (compact_*_many_kernel) against the general Garner kernels
    ("MXX_HIP_SERDE", None): _every(_SERDE_FAST),
    ("MXX_HIP_SERDE", "general"): _every(Expect(ran=("compact_maxbits_kernel",),
                                                absent=("compact_maxbits_fast_kernel", "compact_pack_fast_kernel",
                                                        "compact_maxbits_many_kernel", "compact_pack_many_kernel"))),
    ("MXX_HIP_MUL_SUM_PATH", "tile"): _every(Expect(ran=("matmul_sum_kernel",), absent=("mul_sum_combine_kernel",))),
    ("MXX_HIP_MATMUL_PATH", "reg"): {"u32": _REG},
    ("MXX_HIP_MATMUL_PATH", "lds"): {"u32": Expect(last="matmul_lds_kernel_u32")},
    ("MXX_HIP_MATMUL_PATH", "dma"): {"u32": Expect(last="mmdma::kernel_u32")},
    ("MXX_HIP_MATMUL_PATH", "wide"): {"u32": Expect(last="mmdma32::kernel_u32")},
    ("MXX_HIP_MATMUL_PATH", "mfma"): {"u32": Expect(last="mmfma::kernel_u32")},
    # RCS[p]: matmul_kernel<u32,R,C,S[,loads-ahead]...> (the label of launch_matmul_cfg); the test builds the prefix
    ("MXX_HIP_MATMUL_TILE", "RCS[p]"): {"u32": _REG},
}


class Launched(list):
    """The names of the launches inside a `launches()` block, in launch order (filled when the block ends).  `records` holds
    the trace's own entries in the same order: kernel, blocks (grid x * y * z; 0 for a runtime copy), threads, bytes, ms."""

    records = ()

    def blocks_of(self, prefix):
        """the block counts of the launches whose name starts with `prefix`, in launch order"""
        return [r["blocks"] for r in self.records if r["kernel"].strip().startswith(prefix)]

    @staticmethod
    def word_class(moduli):
        top = max(int(q) for q in moduli)
        return "u32" if top < 1 << 31 else ("u64f" if top.bit_length() <= 51 else "u64")

    def assert_ran(self, switch, value, moduli, forward=False, inverse=False):
        e = TABLE[(switch, value)][self.word_class(moduli)]
        items = e.ran + (e.forward if forward else ()) + (e.inverse if inverse else ())
        assert items, (switch, value, "nothing to assert: say which direction the block transformed")
        for item in items:
            alts = (item,) if isinstance(item, str) else item
            assert any(k.startswith(alts) for k in self), (switch, value, "did not launch", alts, list(self))
        hit = [k for k in self if k.startswith(e.absent)] if e.absent else []
        assert not hit, (switch, value, "launched the other family", hit)


@contextlib.contextmanager
def launches():
    """Syncs the device, traces every launch of the library inside the block and yields the list of their names."""
    names = Launched()
    _ffi.gpu_device_sync()
    _ffi.trace_begin()
    try:
        yield names
    finally:
        names.records = _ffi.trace_end()
        names.extend(t["kernel"].strip() for t in names.records)
