"""CPU-only: the line bench.py prints for the driver and the versioning of the counter records behind its rooflines.

Round 4's line was 30 KB; the driver keeps an 8 KB tail of stdout, so nothing of it could be parsed.  The short line is built
from the full record by `bench.short_line`; here it is built from a recorded full record (round 4's, plus every block this
round adds) and held under 4 KB.  The counter records (`profiles/pmc_<workload>.json`) carry the ISA hash of every kernel
they were counted on; a record of another build must be detected and left unused.
"""
import copy
import json
import os

import pytest

import bench
from mxx_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def recorded_full_line():
    with open(os.path.join(ROOT, "profiles", "r04_bench_default.json")) as f:
        full = json.load(f)
    # the blocks added after that record, shaped as bench.py builds them
    m4 = copy.deepcopy(full["chain_m4"])
    m4.update({"requests_in_flight": 16, "speedup_vs_one_request": 5.123456, "value": 36543.21})
    full["chain_m4_batched"] = m4
    ref = copy.deepcopy(full["preimage"])
    ref["vs_extension_sequence"] = 1.3812345
    full["preimage_reference_sequence"] = ref
    full["compact_bytes"] = {"ms_per_step": 4.9123, "value": 1.234e10, "unit": "B/s", "roofline": {"frac": 0.4123}, "payload_bytes": 61234567,
                             "kernel_ms": 1.2345, "d2h_ms": 2.3456, "pcie_GBps": 26.1234, "host_ms": 0.1234}
    full["gate_batch"] = {"ms_per_step": 0.082123, "value": 195123.4, "unit": "products/s", "roofline": {"frac": 0.2123},
                          "loop_ms": 0.463123, "speedup_vs_loop": 5.64123}
    full["preimage_mixed_keys"] = {"ms_per_step": 2.1234, "value": 30123.4, "unit": "preimages/s", "roofline": {"frac": None},
                                   "requests_in_flight": 16, "loop_ms": 4.81234, "speedup_vs_loop": 2.2661}
    full["sustained"] = {"steps": 8621, "seconds": 5.0123456, "ms_per_step": 0.58141234, "value": 6191234.5}
    full["roofline"]["counters_stale"] = False
    for blk in (full["preimage"], full["preimage_m3b"], full["chain_m4"], full["chain_m4_batched"]):
        blk["roofline"].update({"frac_useful": 0.3123, "lane_utilisation": 0.4212, "counters_stale": False})
    return full


def test_short_line_fits_the_drivers_tail_and_keeps_the_contract_keys():
    full = recorded_full_line()
    assert len(json.dumps(full)) > 20000  # the record that broke round 4's parse
    line = bench.short_line(full)
    text = json.dumps(line)
    assert len(text) < 4096, len(text)
    assert "\n" not in text
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["metric"] == "dcrt_ring_ops_per_s" and line["unit"] == "ring-ops/s" and line["vs_baseline"] is None
    assert line["config"]["workload"].startswith("M2A") and "model" not in line["config"]
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"], rel=1e-3)
    assert rf["traffic"] and rf["algorithmic_bytes_per_launch"] and rf["kernel_ms"]
    cb = line["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 16 and cb["value"] > 0 and cb["sample"]
    assert line["value"] == pytest.approx(full["value"], rel=1e-6) and line["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
    # one record per BASELINE configuration (+ the three the round-4 review asked for, + the batched chain)
    assert set(line["configs"]) == {"m1_ntt_mul", "m2b_product", "m2b_decompose", "m2b_mul_decompose", "m3a_preimage",
                                    "m3a_reference_sequence", "m3b_preimage", "m4_chain", "m4_chain_batched", "m4_mixed_keys",
                                    "compact_bytes", "gate_batch"}
    for name, rec in line["configs"].items():
        assert rec["ms_per_step"] and rec["value"] and rec["unit"], name
    assert line["configs"]["m3a_preimage"]["frac_useful"] == 0.3123
    assert line["configs"]["m4_chain_batched"]["requests"] == 16 and "sustained" in line and "detail" in line
    assert "counters_stale" not in line["configs"]["m3a_preimage"]  # reported only when true
    assert line["configs"]["m1_ntt_mul"]["ntt_frac"] == full["kernels"]["ntt_forward"]["frac_of_hbm_peak"]


def test_short_line_sheds_detail_rather_than_outgrowing_the_limit():
    full = recorded_full_line()
    full["config"]["workload"] = "M2A " + "x" * 4000
    full["config"]["sharding"] = "y" * 4000
    for i in range(40):  # far more blocks than any run produces
        full[f"extra{i}"] = full["chain_m4"]
    line = bench.short_line(full)
    assert len(json.dumps(line)) <= bench.SHORT_LINE_LIMIT
    assert line["roofline"]["frac"] and line["cpu_baseline"]["value"]


def test_short_line_at_n_gpus_carries_the_exchange_verdict():
    full = recorded_full_line()
    full["n_gpus"] = 2
    full["cpu_baseline"] = None
    full["exchange"] = {"ranks_seen": 2, "comm_backend": "torch.distributed 'nccl' (RCCL)", "devices": [0, 1], "peer_access": [[1, 1], [1, 1]],
                        "foreign_blocks_checked_per_rank": [1, 1], "self_validated": True, "distinct_devices": True,
                        "comm_verified_on_distinct_devices_before_this_run": False, "comm_verified_by_this_run": True}
    full["preimage"]["exchange"] = dict(full["exchange"])
    full["gather"] = "step"
    full["other_gather"] = {"gather": "lazy", "ms_per_step": 0.0912345, "value": 39458123.4}
    full["independent_units"] = {"scaling": "weak", "value": 12345678.9, "ms_per_step": 0.5912345, "units_per_step": 7200, "sharding": "x"}
    line = bench.short_line(full)
    assert line["gather"] == "step" and line["other_gather"] == {"gather": "lazy", "value": 39458000, "ms_per_step": 0.091234}
    assert line["independent_units"]["scaling"] == "weak" and line["independent_units"]["value"] == 12346000
    assert line["exchange"] == {"ranks_seen": 2, "comm_backend": "torch.distributed 'nccl' (RCCL)", "self_validated": True,
                                "distinct_devices": True, "comm_verified_by_this_run": True, "preimage_self_validated": True}
    assert line["cpu_baseline"] is None
    assert len(json.dumps(line)) < 4096


def test_dry_run_objects_pass_through():
    assert bench.short_line({"dry_run": True, "world": 2}) == {"dry_run": True, "world": 2}


def test_sig_rounds_to_significant_digits():
    assert bench.sig(6134688.61730078, 7) == 6134689.0
    assert bench.sig(0.5868268504855223, 6) == 0.586827
    assert bench.sig(13.509383658328908) == 13.509
    assert bench.sig(None) is None and bench.sig(26) == 26 and bench.sig(True) is True and bench.sig(0.0) == 0.0


# ---------------------------------------------------------------------------------------------------
# versioned counter records
# ---------------------------------------------------------------------------------------------------
def test_library_kernels_have_isa_hashes():
    h = codeobj.kernel_isa_hashes()
    for k in ("matmul_kernel", "mmdma32::kernel_u32", "ntt14::fwd_kernel", "ntt14::inv_kernel", "ntt14::fwd_digits_kernel",
              "gauss_samp_lanes_kernel", "sample_gauss_kernel", "p1_sample_lanes_kernel", "elementwise_kernel", "*"):
        assert k in h and len(h[k]) == 16, k
    assert codeobj.kernel_isa_hashes() is h  # cached per (path, mtime)
    assert codeobj.kernel_base("void ntt14::fwd_kernel<unsigned int, false>(unsigned int*, int)") == "ntt14::fwd_kernel"
    assert codeobj.kernel_base("(ntt14::fwd_kernel<W, TIGHT>)") == "ntt14::fwd_kernel"


def test_a_counter_record_of_another_build_is_detected(tmp_path, monkeypatch):
    cur = codeobj.kernel_isa_hashes()
    rec = {"workload": "m2a", "steps": 3, "head": "abc1234", "gpupoly_version": "x", "source": "test",
           "kernels": {"matmul_kernel": {"launches_per_step": 1.0, "isa_hash": cur["matmul_kernel"], "hbm_bytes_per_launch": 3.69e9,
                                         "SQ_INSTS_VALU": 3.0e7},
                       "ntt14::fwd_kernel": {"launches_per_step": 1.0, "isa_hash": "0123456789abcdef", "hbm_bytes_per_launch": 1.0,
                                             "SQ_INSTS_VALU": 1.0},
                       "elementwise_kernel": {"launches_per_step": 1.0, "hbm_bytes_per_launch": 1.0, "SQ_INSTS_VALU": 1.0}}}
    prof = tmp_path / "profiles"
    prof.mkdir()
    (prof / "pmc_m2a.json").write_text(json.dumps(rec))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    got = bench.load_counters("m2a")
    assert got["file"] == "profiles/pmc_m2a.json" and got["head"] == "abc1234"
    assert got["kernels"]["matmul_kernel"]["stale"] is False
    assert got["kernels"]["ntt14::fwd_kernel"]["stale"] is True       # counted on other ISA text
    assert got["kernels"]["elementwise_kernel"]["stale"] is True      # no hash at all (a round-4 record)
    assert got["stale_kernels"] == ["elementwise_kernel", "ntt14::fwd_kernel"]
    assert bench.load_counters("m3a") is None
    assert codeobj.stale_kernels({"matmul_kernel": cur["matmul_kernel"], "ntt14::fwd_kernel": "0" * 16}) == ["ntt14::fwd_kernel"]
    assert codeobj.stale_kernels(None) == ["*"]


def test_round4_records_without_hashes_count_as_stale():
    rec = bench.load_counters("m2a", current_hashes=codeobj.kernel_isa_hashes())
    if rec is None or rec["file"].endswith("/pmc_m2a.json"):
        pytest.skip("a versioned record exists; the round-4 fallback is not in use")
    assert rec["file"] == "profiles/r04_pmc_m2a.json" and rec["kernels"]["matmul_kernel"]["stale"] is True


def test_committed_counter_records_match_the_library_or_are_flagged():
    """every versioned record under profiles/ either matches today's kernels or bench.py will say `counters_stale`; the
    valu-mix prices follow the same rule (entries of other builds are dropped)"""
    cur = codeobj.kernel_isa_hashes()
    for wl in ("m1", "m2a", "m2b", "m2b_decompose", "m2b_mul_decompose", "m3a", "m3b", "m4"):
        rec = bench.load_counters(wl, current_hashes=cur)
        if rec is None:
            continue
        for base, k in rec["kernels"].items():
            if base.startswith("__amd_rocclr"):
                continue  # the HIP runtime's copy kernels
            assert k["stale"] == (k.get("isa_hash") is None or k["isa_hash"] != cur.get(base))
    mix = bench.load_valu_mix(cur)
    for base, k in mix.items():
        assert k["isa_hash"] == cur[base] and 2.5 <= k["cycles_per_inst"] <= 4.5


# ---------------------------------------------------------------------------------------------------
# --dump-outputs
# ---------------------------------------------------------------------------------------------------
class _HostMatrix:
    """host stand-in for GpuDCRTPolyMatrix with the members bench.dump_outputs reads"""

    def __init__(self, data, is_ntt=True):
        self.data, self.is_ntt = data, is_ntt
        self.nrow, self.ncol = data.shape[:2]
        self.level = data.shape[2] - 1

    def to_rns(self):
        return self.data.copy()

    def slice(self, r0, r1, c0, c1):
        return _HostMatrix(self.data[r0:r1, c0:c1], self.is_ntt)


class _HostParams:
    def __init__(self, moduli, n):
        self._moduli, self._n = moduli, n

    def moduli(self):
        return list(self._moduli)

    def ring_dimension(self):
        return self._n


class _HostWorkload:
    def __init__(self, moduli, shape, seed=1):
        import numpy as np

        rows, cols, n = shape
        self.params = _HostParams(moduli, n)
        rng = np.random.default_rng(seed)
        self.data = np.stack([rng.integers(0, q, size=(rows, cols, n), dtype=np.uint64) for q in moduli], axis=2)

    def outputs(self):
        return {"product": _HostMatrix(self.data)}


def test_dump_outputs_writes_the_whole_matrix_exactly_when_it_fits(tmp_path):
    import numpy as np

    wl = _HostWorkload([(1 << 24) - 3, (1 << 23) + 9], (2, 3, 16))
    rec = bench.dump_outputs(wl, str(tmp_path / "out"))
    got = np.load(tmp_path / "out" / "product.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 2, 16)
    assert np.array_equal(got.astype(np.uint64), wl.data)  # 24-bit residues are exact in float32
    assert rec["dtype"] == "float32" and rec["files"]["product.npy"]["shape"] == [2, 3, 2, 16]
    assert "sampled_entries" not in rec["files"]["product.npy"]


def test_dump_outputs_samples_fixed_entries_under_the_limit(tmp_path, monkeypatch):
    import numpy as np

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 10 * 3 * 64 * 8)  # room for 10 of the 48 entries
    wl = _HostWorkload([(1 << 50) - 27, (1 << 40) + 15, (1 << 30) + 3], (4, 12, 64))
    rec = bench.dump_outputs(wl, str(tmp_path / "a"))
    got = np.load(tmp_path / "a" / "product.npy")
    assert got.dtype == np.float64 and got.shape == (10, 3, 64)
    assert os.path.getsize(tmp_path / "a" / "product.npy") <= bench.DUMP_LIMIT_BYTES
    pos = rec["files"]["product.npy"]["sampled_entries"]
    assert len(pos) == 10 and pos == sorted(set(pos))
    for k, p in enumerate(pos):
        assert np.array_equal(got[k].astype(np.uint64), wl.data[p // 12, p % 12])
    # another run (another build) with the same shapes samples the same entries
    rec2 = bench.dump_outputs(_HostWorkload(wl.params.moduli(), (4, 12, 64), seed=2), str(tmp_path / "b"))
    assert rec2["files"]["product.npy"]["sampled_entries"] == pos


def test_steps_and_dump_outputs_arguments_are_checked(capsys):
    args = bench.parse_args(["--steps", "7", "--warmup", "0", "--dump-outputs", "d"])
    assert args.steps == 7 and args.dump_outputs == "d"
    assert bench.parse_args(["--workload", "m2b_decompose", "--dump-outputs", "d"]).workload == "m2b_decompose"
    for bad in (["--steps", "0"], ["--workload", "m3a", "--dump-outputs", "d"], ["--inproc", "--dump-outputs", "d"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)
    capsys.readouterr()


def test_a_plain_run_leaves_the_extras_to_full():
    """A plain run times the headline steps only: no repeats and no sustained region unless asked for; --full brings
    back the defaults of a complete record, and explicit values hold in both modes."""
    plain = bench.parse_args(["--steps", "5", "--warmup", "2"])
    assert plain.full is False and plain.repeats == 0 and plain.sustain == 0.0
    assert plain.steps == 5 and plain.warmup == 2
    full = bench.parse_args(["--full"])
    assert full.full is True and full.repeats == 10 and full.sustain == 5.0
    assert bench.parse_args(["--repeats", "3", "--sustain", "1"]).repeats == 3
    assert bench.parse_args(["--full", "--repeats", "0", "--sustain", "0"]).sustain == 0.0
