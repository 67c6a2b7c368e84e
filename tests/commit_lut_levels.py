"""The rows of the two commit-lookup message entries in the coverage table of matrices below the top level (tests/levels.py,
held against include/gpupoly.h by tests/test_level_table_host.py).  Importing this module puts them into levels.TABLE; both
test modules of the entries import it - the CPU one (tests/test_abi_commit_lut.py) and the GPU one that holds the test the
rows name."""
import levels

LOW = "test_gpu_commit_lut::test_operands_below_the_top_level_equal_the_literal"
ROWS = {"gpupoly_matrix_commit_lut_messages": (LOW,), "gpupoly_matrix_commit_lut_messages_combine": (LOW,)}
for _entry, _row in ROWS.items():
    levels.TABLE.setdefault(_entry, _row)
