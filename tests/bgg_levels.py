"""The rows of the two BGG+ encoding entries in the coverage table of matrices below the top level (tests/levels.py, held
against include/gpupoly.h by tests/test_level_table_host.py).  Importing this module puts them into levels.TABLE; both new
test modules of the entries import it - the CPU one (tests/test_abi_bgg_encode.py, which needs no device and nothing but
the standard library) and the GPU one that holds the test the rows name."""
import levels

LOW = "test_gpu_bgg_encode::test_operands_below_the_top_level_equal_the_plain_reference"
ROWS = {"gpupoly_matrix_bgg_encode_slots": (LOW,), "gpupoly_matrix_bgg_encode_slots_combine": (LOW,)}
for _entry, _row in ROWS.items():
    levels.TABLE.setdefault(_entry, _row)
