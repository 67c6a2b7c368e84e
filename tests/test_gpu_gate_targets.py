"""GPU: the GGH15 gate-stage preimage targets of many gates in one sequence of launches (`mxx_amd.lookup.gate_stage_targets`
and the five stage wrappers) against the reference's per-gate functions restated statement by statement
(`build_gate_stageN_target_chunk`, src/lookup/ggh15/pubkey_gpu.rs:418-537), bit for bit under the same seeds, and the stage's
preimages through the batched preimage entry."""
import numpy as np
import pytest

from conftest import make_params

pytestmark = pytest.mark.gpu

N, DEPTH, BITS, BASE, D = 256, 3, 51, 17, 2
GATES = (7, 3, 12)       # not consecutive
CHUNK = (4, 4)           # four columns, not the first chunk
SIGMAS = (3.5, 0.0)
KEY = bytes((11 * i + 3) & 0xFF for i in range(32))
LUT_ID = 5


def seed_bytes(tag):
    return bytes((tag * 41 + 13 * i + 7) & 0xFF for i in range(32))


def gseed(gpu, tag):
    return gpu.GpuRngSeed.from_bytes(seed_bytes(tag))


def launches(fn):
    from mxx_amd import _ffi

    c0 = _ffi.lib().gpupoly_launch_count()
    fn()
    return _ffi.lib().gpupoly_launch_count() - c0


@pytest.fixture(scope="module")
def world(gpu, oracle):
    """the shared matrices, computed once and left unchanged"""
    from mxx_amd.lookup import GateShared

    p = make_params(gpu, oracle, N, DEPTH, BITS, BASE)
    M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()
    m_g = D * p.modulus_digits()
    assert CHUNK[0] > 0 and CHUNK[0] + CHUNK[1] <= m_g
    res = {name: oracle.random_matrix(300 + i, D, m_g, moduli, N) for i, name in enumerate(("b1", "w_identity", "w_gy", "w_v"))}
    mats = {name: M.from_rns(p, r, True) for name, r in res.items()}
    shared = GateShared(p, KEY, LUT_ID, mats["b1"], mats["w_identity"], mats["w_gy"], mats["w_v"])
    inputs = [M.from_rns(p, oracle.random_matrix(320 + t, D, m_g, moduli, N), True) for t in range(len(GATES))]
    u_gs = [M.from_rns(p, oracle.random_matrix(330 + t, D, m_g, moduli, N), True) for t in range(len(GATES))]
    return dict(p=p, shared=shared, res=res, inputs=inputs, u_gs=u_gs, m_g=m_g)


def seeds_for(gpu, count, base=400):
    return [gseed(gpu, base + t) for t in range(count)], [gseed(gpu, base + 50 + t) for t in range(count)]


def stage_legs(gpu, world, stage, sigma, gates=GATES, base=400):
    """(batched targets, per-gate targets) of one stage"""
    from mxx_amd import lookup as L

    sh, count = world["shared"], len(gates)
    s_seeds, e_seeds = seeds_for(gpu, count, base)
    inputs = [world["inputs"][t % len(GATES)] for t in range(count)]
    u_gs = [world["u_gs"][t % len(GATES)] for t in range(count)]
    if stage == 1:
        batched = L.gate_stage1_targets(sh, s_seeds, e_seeds, sigma, CHUNK)
        alone = [L.build_gate_stage1_target_chunk(sh, s_seeds[t], e_seeds[t], sigma, *CHUNK) for t in range(count)]
    elif stage == 2:
        batched = L.gate_stage2_targets(sh, gates, s_seeds, e_seeds, sigma, CHUNK)
        alone = [L.build_gate_stage2_target_chunk(sh, gates[t], s_seeds[t], e_seeds[t], sigma, *CHUNK) for t in range(count)]
    elif stage == 3:
        batched = L.gate_stage3_targets(sh, s_seeds, e_seeds, sigma, CHUNK)
        alone = [L.build_gate_stage3_target_chunk(sh, s_seeds[t], e_seeds[t], sigma, *CHUNK) for t in range(count)]
    elif stage == 4:
        batched = L.gate_stage4_targets(sh, gates, s_seeds, inputs, e_seeds, sigma, CHUNK)
        alone = [L.build_gate_stage4_target_chunk(sh, gates[t], s_seeds[t], inputs[t], e_seeds[t], sigma, *CHUNK) for t in range(count)]
    else:
        batched = L.gate_stage5_targets(sh, s_seeds, u_gs, e_seeds, sigma, CHUNK)
        alone = [L.build_gate_stage5_target_chunk(sh, s_seeds[t], u_gs[t], e_seeds[t], sigma, *CHUNK) for t in range(count)]
    return batched, alone


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("stage", [1, 2, 3, 4, 5])
def test_batched_targets_equal_the_per_gate_restatement(gpu, oracle, world, stage, sigma):
    batched, alone = stage_legs(gpu, world, stage, sigma)
    assert len(batched) == len(alone) == len(GATES)
    for t in range(len(GATES)):
        assert batched[t].size() == (D, CHUNK[1]) and batched[t].is_ntt
        assert batched[t] == alone[t], (stage, sigma, t)
    assert not (batched[0] == batched[1])  # the gates' targets differ: nobody compared a matrix with itself


@pytest.mark.parametrize("sigma", SIGMAS)
def test_stage1_equals_the_oracle_pieces(gpu, oracle, world, sigma):
    """S and E from the CPU restatement of the samplers, the product from the oracle: not only the GPU's older entries"""
    p, moduli = world["p"], world["p"].moduli()
    batched, alone = stage_legs(gpu, world, 1, sigma)
    w = world["res"]["b1"][:, CHUNK[0]:CHUNK[0] + CHUNK[1]]
    for t in range(len(GATES)):
        s = oracle.matrix_ntt(oracle.sample_distribution(D, D, moduli, N, "ternary", 0.0, seed_bytes(400 + t)), moduli)
        want = oracle.matmul(s, w, moduli)
        if sigma:
            e = oracle.matrix_ntt(oracle.sample_distribution(D, CHUNK[1], moduli, N, "gauss", sigma, seed_bytes(450 + t)), moduli)
            want = oracle.pointwise("add", want, e, moduli)
        assert np.array_equal(alone[t].to_rns(), want) and np.array_equal(batched[t].to_rns(), want), t


@pytest.mark.parametrize("stage", [1, 3])
def test_the_launches_do_not_depend_on_the_gate_count(gpu, oracle, world, stage):
    from mxx_amd import lookup as L

    sh = world["shared"]
    fn = L.gate_stage1_targets if stage == 1 else L.gate_stage3_targets
    build = L.build_gate_stage1_target_chunk if stage == 1 else L.build_gate_stage3_target_chunk
    counts = {}
    for count in (2, 16):
        s_seeds, e_seeds = seeds_for(gpu, count, 500)
        counts[count] = launches(lambda: fn(sh, s_seeds, e_seeds, 3.5, CHUNK))
    loop = launches(lambda: [build(sh, s, e, 3.5, *CHUNK) for s, e in zip(s_seeds, e_seeds)])
    print(f"stage {stage}: launches for 2 gates {counts[2]}, for 16 gates {counts[16]}, per-gate loop over 16 gates {loop}")
    assert counts[2] == counts[16] and 0 < counts[16] < loop
    batched, alone = stage_legs(gpu, world, stage, 3.5, gates=tuple(range(16)), base=500)
    assert all(b == a for b, a in zip(batched, alone))


def test_stage3_preimages_through_the_batched_entry(gpu, oracle, world):
    from mxx_amd import lookup as L

    p, sh = world["p"], world["shared"]
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, 4.578)
    td, pub = sampler.trapdoor(p, D)
    s_seeds, e_seeds = seeds_for(gpu, len(GATES))
    triples = [tuple(gseed(gpu, 600 + 3 * t + i) for i in range(3)) for t in range(len(GATES))]
    targets = L.gate_stage3_targets(sh, s_seeds, e_seeds, 3.5, CHUNK)
    pairs = L.sample_gate_preimages(sh, sampler, td, pub, targets, _seeds=triples)
    assert len(pairs) == len(GATES)
    for t, (target, x) in enumerate(pairs):
        alone_target = L.build_gate_stage3_target_chunk(sh, s_seeds[t], e_seeds[t], 3.5, *CHUNK)
        assert target == alone_target, t  # the batched preimage left its inputs alone
        assert pub * x == target, t
        assert x == sampler.preimage(p, td, pub, alone_target, _seeds=triples[t]), t
