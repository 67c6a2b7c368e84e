"""GPU: the Wee25 commitment over public parameters built with the batched target call (mxx_amd/commit.py; DESIGN.md section
5v) - the reference's own acceptance tests (src/commit/wee25.rs:1270-1525) at the smallest ring the batched preimage serves:
n = 128, two 24-bit limbs with four digits (base 2^12), secret_size = 1, tree_base = 2, four message blocks.  That is 48
indices x 8 parts = 384 targets in six waves of eight indices, each one target call and one preimage call.  The parameters are
built once and shared; every predicate is exact (`==` on canonical residues)."""
import pytest

from conftest import make_params
from test_gpu_preimage_abi import explicit_seeds, seed_bytes, trapdoor_and_oracle

pytestmark = pytest.mark.gpu

N, DEPTH, BITS, BASE = 128, 2, 24, 12
SECRET, TREE_BASE, COLS, SIGMA = 1, 2, 4, 4.578
KEY = bytes((7 * i + 1) & 0xFF for i in range(32))
_STATE = {}


def state(gpu, oracle):
    """(Wee25Commit, setup = (trapdoor, b, t_bottom), seeds per (idx, col_start), the parameters built in waves of eight)"""
    from mxx_amd.commit import Wee25Commit

    if not _STATE:
        p = make_params(gpu, oracle, N, DEPTH, BITS, BASE)
        w = Wee25Commit(p, SECRET, TREE_BASE, SIGMA)
        assert (w.log_base_q, w.m_g, w.m_b, w.pp_size, w.nparts) == (4, 4, 6, 48, 8)
        _, td, b, _ = trapdoor_and_oracle(gpu, oracle, p, N, BASE, SECRET, seed_bytes(21))
        t_bottom = gpu.GpuDCRTPolyUniformSampler().sample_uniform(p, w.m_b, w.j_2m_cols, gpu.DistType.GaussDist(SIGMA))
        keys = [(idx, c) for idx in range(w.pp_size) for c in range(0, w.j_2m_cols, w.m_b)]
        seeds = dict(zip(keys, explicit_seeds(gpu, len(keys), 4000)))
        setup = (td, b, t_bottom)
        calls = []
        abi = gpu.GpuDCRTPolyTrapdoorSampler.preimage_many_abi

        def counted(self, params, td_, a, targets, _seeds=None):
            calls.append(len(targets))
            return abi(self, params, td_, a, targets, _seeds=_seeds)

        gpu.GpuDCRTPolyTrapdoorSampler.preimage_many_abi = counted
        try:
            pp = w.sample_public_params(KEY, batch=8, _setup=setup, _seeds=seeds)
        finally:
            gpu.GpuDCRTPolyTrapdoorSampler.preimage_many_abi = abi
        assert calls == [64] * 6  # six preimage calls of 8 indices x 8 parts
        _STATE.update(w=w, setup=setup, seeds=seeds, pp=pp)
    return _STATE["w"], _STATE["setup"], _STATE["seeds"], _STATE["pp"]


def message(gpu, oracle, w, seed):
    p = w.params
    return [gpu.GpuDCRTPolyMatrix.from_rns(p, oracle.random_matrix(seed + j, SECRET, w.m_b, p.moduli(), N), True) for j in range(COLS)]


def concat(blocks):
    return blocks[0].concat_columns(blocks[1:])


def test_public_params_are_preimages_of_the_targets(gpu, oracle):
    w, (td, b, t_bottom), _, pp = state(gpu, oracle)
    assert len(pp.t_top) == 384 and len(pp.t_bottom_parts) == 8 and pp.hash_key == KEY and pp.b is b
    sample = [0, 5, 17, 30, 47]
    targets = w.t_top_target_blocks(t_bottom, sample)
    for t, idx in enumerate(sample):
        for part in range(w.nparts):
            block = pp.t_top[(idx, part * w.m_b)]
            assert block.size() == (w.m_b, w.m_b)
            assert b * block == targets[t][part], (idx, part)
            if part in (0, 7):  # and the literal leg agrees
                assert targets[t][part] == w.t_top_target_block(idx, part * w.m_b, pp.t_bottom_parts[part]), (idx, part)


def test_commit_base_equals_its_literal_loop(gpu, oracle):
    w, _, _, pp = state(gpu, oracle)
    msg = concat(message(gpu, oracle, w, 300)[:TREE_BASE])
    assert w.commit_base(msg, pp) == w.commit_base_literal(msg, pp)


@pytest.mark.parametrize("kind", ["zero", "random"])
def test_commit_open_verify(gpu, oracle, kind):
    """test_wee25_zero_commit_verify, test_wee25_random_commit_verify (:1270-1387)"""
    w, _, _, pp = state(gpu, oracle)
    M = gpu.GpuDCRTPolyMatrix
    blocks = [M.zero(w.params, SECRET, w.m_b) for _ in range(COLS)] if kind == "zero" else message(gpu, oracle, w, 100)
    cache = {}
    commitment = w.commit(blocks, pp, cache)
    assert commitment.size() == (SECRET, w.m_b) and set(cache) == {(0, 2), (2, 2), (0, 4)}
    opening = w.open(blocks, None, pp, cache)
    assert w.verify(concat(blocks), commitment, opening, None, pp)


def test_a_changed_message_does_not_verify(gpu, oracle):
    """test_wee25_random_invalid_commit_verify (:1389-1454): the commitment of one message, the opening of another"""
    w, _, _, pp = state(gpu, oracle)
    blocks1 = message(gpu, oracle, w, 100)
    blocks2 = [b.clone() for b in blocks1]
    blocks2[0].set_entry(0, 0, blocks2[0].entry(0, 0) + gpu.GpuDCRTPoly.const_one(w.params))
    cache = {}
    commitment = w.commit(blocks1, pp, cache)
    opening = w.open(blocks2, None, pp, cache)
    assert not w.verify(concat(blocks2), commitment, opening, None, pp)
    assert w.verify(concat(blocks1), commitment, w.open(blocks1, None, pp, cache), None, pp)


def test_partial_opening_verifies(gpu, oracle):
    """test_wee25_random_partial_open_verify (:1456-1524): col_range = 1..3"""
    w, _, _, pp = state(gpu, oracle)
    blocks = message(gpu, oracle, w, 200)
    cache = {}
    commitment = w.commit(blocks, pp, cache)
    col_range = range(1, 3)
    opening = w.open(blocks, col_range, pp, cache)
    assert w.verify(concat(blocks), commitment, opening, col_range, pp)
    assert not w.verify(concat(blocks), commitment, opening, range(0, 2), pp)


def test_waves_of_five_equal_one_index_at_a_time(gpu, oracle):
    w, setup, seeds, pp = state(gpu, oracle)
    five = w.sample_public_params(KEY, batch=5, _setup=setup, _seeds=seeds)
    one = w.sample_public_params(KEY, batch=1, as_bytes=True, _setup=setup, _seeds=seeds)
    assert set(five.t_top) == set(one.t_top) == set(pp.t_top) and len(one.t_top) == 384
    blobs = [one.t_top[key] for key in sorted(one.t_top)]
    assert all(isinstance(blob, bytes) for blob in blobs) and all(isinstance(part, bytes) for part in one.t_bottom_parts)
    loaded = gpu.GpuDCRTPolyMatrix.from_compact_bytes_many(w.params, blobs)
    for key, block in zip(sorted(one.t_top), loaded):
        assert five.t_top[key] == pp.t_top[key], key
        assert block.ensure_eval() == pp.t_top[key], key
