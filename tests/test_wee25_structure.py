"""CPU-only, no library call: the closed form `Wee25Commit.j_2m_hit` against the index arithmetic of build_j_2m_block
(src/commit/wee25.rs:549-575) restated as a plain loop, for every public-parameter index of every small shape, and the W
block tags against the reference's bytes (:693-695)."""
import pytest


class _Params:
    """what Wee25Commit reads of its parameters when nothing is computed"""

    def __init__(self, k):
        self.k = k

    def modulus_digits(self):
        return self.k


def literal_hits(idx, s, k, m_g):
    """[(row i, gadget index of the coefficient, [global columns])] of the rows build_j_2m_block writes entries into"""
    block_group = idx // m_g
    out = []
    for i in range(s):
        r = idx * s + i
        r_g_start = r * k
        slice_start = block_group * m_g * m_g
        offset = r_g_start - slice_start
        step = m_g + 1
        c = (offset + step - 1) // step
        if c < m_g:
            pos = slice_start + c * step
            if pos <= r_g_start + k - 1:
                out.append((i, pos - r_g_start, [block_group * k + sp for sp in range(k)]))
    return out


@pytest.mark.parametrize("tree_base", [2, 3])
@pytest.mark.parametrize("k", [1, 2, 4, 5])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_the_hit_of_every_index_equals_the_literal_arithmetic(s, k, tree_base):
    from mxx_amd.commit import Wee25Commit

    w = Wee25Commit(_Params(k), s, tree_base, 4.578)
    assert (w.m_g, w.m_b) == (s * k, s * (k + 2))
    assert w.pp_size == tree_base * w.m_b * w.m_g and w.j_2m_cols == tree_base * w.m_b * k and w.nparts == tree_base * k
    seen = set()
    for idx in range(w.pp_size):
        hits = literal_hits(idx, s, k, w.m_g)
        assert len(hits) == 1, (idx, hits)  # exactly one row is non-zero
        i, kk, cols = hits[0]
        i_star, kk_closed, first = w.j_2m_hit(idx)
        assert (i_star, kk_closed) == (i, kk) and cols == list(range(first, first + k)), idx
        assert cols[-1] < w.j_2m_cols
        seen.add((i, kk, first))
    assert len(seen) == w.pp_size  # every index has its own (row, digit, column group)


def test_tags_equal_the_reference_bytes():
    from mxx_amd import IndexedTags
    from mxx_amd.commit import Wee25Commit

    assert Wee25Commit.tag(0) == b"wee25_w_block_" + bytes(8)
    assert Wee25Commit.tag(0x0102030405060708) == b"wee25_w_block_\x08\x07\x06\x05\x04\x03\x02\x01"
    tags = Wee25Commit.tags(255, 3)
    assert isinstance(tags, IndexedTags) and not tags.decimal and tags.prefix == b"wee25_w_block_"
    assert list(tags) == [Wee25Commit.tag(i) for i in (255, 256, 257)]
    assert list(tags)[1] == b"wee25_w_block_\x00\x01" + bytes(6)
