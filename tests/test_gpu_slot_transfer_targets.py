"""GPU: the slot-transfer gate preimage targets of a wave of requests in a number of launches that does not depend on the wave
(`mxx_amd.slot_transfer.gate_target_chunks`, `slot_reduce_gate_target_chunks`) against the reference's per-request functions
restated literally (`build_gate_target_chunk`, `build_slot_reduce_gate_target_chunk`; src/slot_transfer/bgg_pubkey_gpu.rs:
371-407,409-471), bit for bit under the same seeds, and the wave's preimages through the batched preimage entry."""
import ctypes as C

import pytest

from conftest import make_params

pytestmark = pytest.mark.gpu

N = 256
RINGS = {"2x51bit": (2, 51, 17), "2x24bit": (2, 24, 12)}  # depth, limb bits, base bits
CHUNK_WIDTH = {12: 5, 8: 3, 6: 4, 4: 3}  # by m_g: first, middle and a narrower last chunk at secret_size 2; first and narrower last at 1
SIGMAS = (0.0, 4.578)
KEY = bytes((7 * i + 5) & 0xFF for i in range(32))
GATE = 9
MAX_T, MAX_SLOTS = 17, 8


def gseed(gpu, tag):
    return gpu.GpuRngSeed.from_bytes(bytes((tag * 37 + 11 * i + 3) & 0xFF for i in range(32)))


def raw_same(a, b) -> bool:
    """gpu_matrix_equal on the handles: residues AND format tag"""
    from mxx_amd import _ffi

    eq = C.c_int(0)
    _ffi.check_status(_ffi.lib().gpu_matrix_equal(a.raw, b.raw, C.byref(eq)), "gpu_matrix_equal")
    return bool(eq.value)


def launches(fn):
    from mxx_amd import _ffi

    c0 = _ffi.lib().gpupoly_launch_count()
    fn()
    return _ffi.lib().gpupoly_launch_count() - c0


def chunks(m_g):
    w = CHUNK_WIDTH[m_g]
    return [(c0, min(w, m_g - c0)) for c0 in range(0, m_g, w)]


_worlds = {}


def world(gpu, oracle, ring, d):
    """the operands of one ring and secret size, made once and left unchanged"""
    if (ring, d) not in _worlds:
        from mxx_amd.slot_transfer import SlotGateShared

        depth, bits, base = RINGS[ring]
        p = make_params(gpu, oracle, N, depth, bits, base)
        M, moduli = gpu.GpuDCRTPolyMatrix, p.moduli()
        m_g = d * p.modulus_digits()
        rnd = lambda seed, rows, cols, ev=True: M.from_rns(p, oracle.random_matrix(seed, rows, cols, moduli, N), ev)  # noqa: E731
        w = dict(p=p, d=d, m_g=m_g, shared=SlotGateShared(p, KEY, d))
        w["lhs_inputs"] = [rnd(1000 + t, d, m_g) for t in range(MAX_T)]
        w["s_js"] = [rnd(1100 + t, d, d) for t in range(MAX_T)]
        w["a_js"] = [rnd(1200 + t, d, m_g, ev=t % 2 == 0) for t in range(MAX_T)]  # public keys in either form
        w["scalars"] = [rnd(1300 + t, 1, 1) if t % 3 != 1 else None for t in range(MAX_T)]
        w["e_seeds"] = [gseed(gpu, 1400 + t) for t in range(MAX_T)]
        w["slot_secrets"] = [rnd(1500 + s, d, d) for s in range(MAX_SLOTS)]
        w["slot_as"] = [rnd(1600 + s, d, m_g, ev=s % 3 != 2) for s in range(MAX_SLOTS)]
        w["a_ins"] = [rnd(1700 + i, d, m_g) for i in range(2)]
        _worlds[(ring, d)] = w
    return _worlds[(ring, d)]


@pytest.mark.parametrize("count", [1, 3, 17])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("ring", list(RINGS))
def test_gate_targets_equal_the_per_request_restatement(gpu, oracle, ring, d, count):
    from mxx_amd import slot_transfer as ST

    w = world(gpu, oracle, ring, d)
    sh = w["shared"]
    args = [w[name][:count] for name in ("lhs_inputs", "s_js", "a_js", "scalars", "e_seeds")]
    assert count == 1 or any(s is None for s in args[3]) and any(s is not None for s in args[3])
    for chunk in chunks(w["m_g"]):
        for sigma in SIGMAS:
            batched = ST.gate_target_chunks(sh, GATE, *args[:4], args[4], sigma, chunk)
            assert len(batched) == count
            for t in range(count):
                alone = ST.build_gate_target_chunk(sh, GATE, args[0][t], args[1][t], args[2][t], args[3][t], args[4][t], sigma, *chunk)
                assert batched[t].size() == (d, chunk[1]) and raw_same(batched[t], alone), (chunk, sigma, t)
    for t, a in enumerate(args[2]):  # the public keys keep their form
        assert a.is_ntt == (t % 2 == 0)


@pytest.mark.parametrize("shared_input", [True, False], ids=["one_input", "two_inputs"])
@pytest.mark.parametrize("num_slots", [3, 8])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("ring", list(RINGS))
def test_slot_reduce_targets_equal_the_per_request_restatement(gpu, oracle, ring, d, num_slots, shared_input):
    from mxx_amd import slot_transfer as ST

    w = world(gpu, oracle, ring, d)
    sh = w["shared"]
    secrets, slot_as = w["slot_secrets"][:num_slots], w["slot_as"][:num_slots]
    dst_slots = list(range(num_slots))[::-1]  # one request per destination slot
    a_ins = [w["a_ins"][0 if shared_input else t % 2] for t in range(num_slots)]
    e_seeds = w["e_seeds"][:num_slots]
    cs = chunks(w["m_g"])
    for chunk, sigma in ((cs[0], SIGMAS[1]), (cs[-1], SIGMAS[0]), (cs[len(cs) // 2], SIGMAS[1])):
        batched = ST.slot_reduce_gate_target_chunks(sh, GATE, a_ins, dst_slots, secrets, slot_as, e_seeds, sigma, chunk)
        for t in range(num_slots):
            alone = ST.build_slot_reduce_gate_target_chunk(sh, GATE, a_ins[t], dst_slots[t], secrets, slot_as, e_seeds[t], sigma, *chunk)
            assert raw_same(batched[t], alone), (chunk, sigma, t)


def test_the_launches_do_not_depend_on_the_request_count(gpu, oracle):
    from mxx_amd import slot_transfer as ST

    w = world(gpu, oracle, "2x51bit", 2)
    sh, chunk = w["shared"], chunks(w["m_g"])[1]
    gate, reduce_ = {}, {}
    for count in (2, 17):
        args = [w[name][:count] for name in ("lhs_inputs", "s_js", "a_js", "scalars", "e_seeds")]
        gate[count] = launches(lambda: ST.gate_target_chunks(sh, GATE, *args[:4], args[4], 4.578, chunk))
        dst = [(t + 1) % MAX_SLOTS for t in range(count)]  # slots 1 and 2 first: public keys of both forms at either count
        a_ins = [w["a_ins"][t % 2] for t in range(count)]
        reduce_[count] = launches(lambda: ST.slot_reduce_gate_target_chunks(sh, GATE, a_ins, dst, w["slot_secrets"], w["slot_as"], args[4], 4.578, chunk))
    loop = launches(lambda: [ST.build_gate_target_chunk(sh, GATE, *(w[name][t] for name in ("lhs_inputs", "s_js", "a_js", "scalars", "e_seeds")),
                                                        4.578, *chunk) for t in range(17)])
    print(f"gate form: {gate[2]} launches for 2 requests, {gate[17]} for 17, per-request loop over 17: {loop}; "
          f"reduce form with 8 slots: {reduce_[2]} for 2, {reduce_[17]} for 17")
    assert gate[2] == gate[17] and 0 < gate[17] < loop
    assert reduce_[2] == reduce_[17] and reduce_[17] > 0


def test_preimages_of_the_targets_through_the_batched_entry(gpu, oracle):
    from mxx_amd import slot_transfer as ST

    d, count = 2, 3
    w = world(gpu, oracle, "2x51bit", d)
    p, sh = w["p"], w["shared"]
    chunk = chunks(w["m_g"])[1]
    sampler = gpu.GpuDCRTPolyTrapdoorSampler(p, 4.578)
    td, pub = sampler.trapdoor(p, d)
    args = [w[name][:count] for name in ("lhs_inputs", "s_js", "a_js", "scalars", "e_seeds")]
    triples = [tuple(gseed(gpu, 1800 + 3 * t + i) for i in range(3)) for t in range(count)]
    targets = ST.gate_target_chunks(sh, GATE, *args[:4], args[4], 4.578, chunk)
    pairs = ST.sample_gate_preimages(sh, sampler, td, pub, targets, _seeds=triples)
    assert len(pairs) == count
    for t, (target, x) in enumerate(pairs):
        alone = ST.build_gate_target_chunk(sh, GATE, args[0][t], args[1][t], args[2][t], args[3][t], args[4][t], 4.578, *chunk)
        assert raw_same(target, alone), t  # the batched preimage left its inputs alone
        assert pub * x == target, t
