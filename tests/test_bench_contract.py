"""The bench line's contract (the driver parses it): keys and types of the `roofline` object, built here from the
committed counter summaries without a GPU, and -- on the GPU box -- of the whole line of a short default run."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _fracs(o, path=""):
    """every (path, value) of a key named `frac` anywhere inside o"""
    if isinstance(o, dict):
        for k, v in o.items():
            if k == "frac":
                yield path + "/frac", v
            yield from _fracs(v, path + "/" + k)
    elif isinstance(o, list):
        for i, v in enumerate(o):
            yield from _fracs(v, f"{path}[{i}]")


@pytest.mark.parametrize("name,dom,ms,alg,workload,arith", [("current_pmc.json", "k_mix_levels", 0.0766, 597120000, "config3", 1),
                                                            ("pmc_10k.json", "k_mix_levels", 0.70, 5905536000, "10k", 1),
                                                            ("pmc_flat.json", "k_mix_decimate(level0)", 0.36, 3145728000, "flat", 1),
                                                            ("pmc_config4.json", "k_mix_levels", 0.032, 135840000, "config4", 1),
                                                            ("pmc_config3_tolerance.json", "k_mix_levels", 0.060, 597120000, "config3", 0),
                                                            ("pmc_config3_robust.json", "k_mix_levels", 0.065, 597120000, "config3", 2),
                                                            ("pmc_10k_robust.json", "k_mix_levels", 0.59, 5905536000, "10k", 2),
                                                            ("pmc_config4_robust.json", "k_mix_levels", 0.027, 135840000, "config4", 2)])
def test_roofline_object_keeps_the_contract_keys(name, dom, ms, alg, workload, arith):
    """`frac` is the fraction of the bound that binds (<= 1 by construction), `bound` is that limiter -- never a label that
    disagrees with the counters -- and SURVEY 8d's algorithmic figure, which may exceed the peak, is not called a fraction."""
    b = _bench()
    pm = json.load(open(os.path.join(ROOT, "profiles", name)))
    assert int(pm["exact"]) == arith and pm["workload"] == workload and pm is not None and b.pmc_for(workload, arith)["source"] == pm["source"]
    if dom not in pm["kernels"]:
        dom = next(k for k in pm["kernels"] if k.startswith("k_mix"))
    from sdrreceiver_amd import topology as tp
    topo = {"config3": lambda: tp.config3(1024), "10k": lambda: tp.config3(10240), "flat": lambda: tp.config3_flat(1024),
            "config4": lambda: tp.config4(256)}[workload]()
    r = b.roofline_object(dom, {"alg_bytes": alg * 20, "launches": 20, "ms": ms * 20}, 20, 2 * ms, alg, 1, pm, 70000,
                          b.demanded_valu_per_launch(topo, arith))
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_GBps", "frac_hbm_unique"):
        assert k in r, k
    assert r["bound"] in ("hbm", "valu") and r["bound"] == r["limiter"]
    assert abs(r["algorithmic_GBps"] - alg / (ms * 1e-3) / 1e9) < 1.0
    assert 0.0 < r["frac"] <= 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 2e-3
    assert 0.0 < r["frac_hbm_unique"] <= 1.0
    for path, v in _fracs(r):
        assert v is None or 0.0 <= v <= 1.0, (path, v)
    if r["bound"] == "hbm":
        assert r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["frac"] == r["frac_hbm_unique"] >= r["valu"]["busy"]
    else:
        # `peak` comes from the hardware (1024 SIMDs, the pass's clock) and the calibration probe alone, `achieved` from the
        # instruction counters over the dispatch's duration: their ratio must agree with the calibrated busy reading, which
        # is derived from the cycle counter instead -- a check of one against the other, not an identity
        v = r["valu"]
        assert abs(r["peak"] - 1024 * v["clock_GHz"] / 4.0 * v["probe_reads_raw"]) < 0.1
        assert abs(r["frac"] - v["busy"]) < 0.02 and r["frac"] > r["frac_hbm_unique"]
    assert isinstance(r["traffic"], int) and r["traffic"] > 0
    v = r["valu"]
    assert 0.0 < v["busy"] <= 1.0 and 0.0 < v["useful_frac"] <= v["busy"] and v["demanded_insts_per_launch"] <= v["issued_insts_per_launch"] * 1.5


def test_roofline_object_without_counters_claims_nothing():
    b = _bench()
    r = b.roofline_object("k_mix_levels", {"alg_bytes": 6e9, "launches": 10, "ms": 0.7}, 10, 0.1, 6e8, 1, None, 1000)
    assert r["bound"] is None and r["frac"] is None and r["algorithmic_GBps"] > 8000 and "unknown" in r["limited_by"]


def test_no_committed_kernel_reads_more_than_fully_busy():
    """the calibrated VALU reading of every kernel of every committed counter summary is a
    fraction, and every probe of the calibration run reads 0.94-0.98 raw (1.00 +- 0.03 after the division by the
    mix-matched probe)."""
    cal = json.load(open(os.path.join(ROOT, "profiles", "valu_calibration.json")))["probes"]
    assert len(cal) == 13
    for name, p in cal.items():
        assert 0.93 <= p["valu_busy_raw"] <= 0.99, (name, p)
    for f in sorted(n for n in os.listdir(os.path.join(ROOT, "profiles")) if n.endswith("_pmc.json") or n.startswith("pmc_")):
        pm = json.load(open(os.path.join(ROOT, "profiles", f)))
        for k, e in pm["kernels"].items():
            if "valu" in e:
                assert 0.0 <= e["valu"].get("valu_busy", e["valu"]["valu_busy_raw"]) <= 1.0, (f, k)


def test_counter_summaries_know_every_kernel_of_the_committed_traces():
    """tools/pmc_summary.py maps demangled kernel names to the keys bench.py looks up; round 6 added a template parameter to
    k_mix_decimate and the flat workload's dominant kernel silently fell out of its summary.  Every kernel of the product in the
    committed round-6 traces must map, and every summary must hold the dominant kernel of its workload."""
    import csv
    spec = importlib.util.spec_from_file_location("pmc_summary", os.path.join(ROOT, "tools", "pmc_summary.py"))
    ps = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ps)
    seen = set()
    for d in sorted(n for n in os.listdir(os.path.join(ROOT, "profiles")) if n.startswith("r06") and os.path.exists(os.path.join(ROOT, "profiles", n, "kernel_stats.csv"))):
        for r in csv.DictReader(open(os.path.join(ROOT, "profiles", d, "kernel_stats.csv"))):
            if "sdrx::k_" in r["Name"] and "k_nco_init" not in r["Name"]:
                assert ps.key_of(r["Name"]) is not None, (d, r["Name"])
                seen.add(ps.key_of(r["Name"]))
    assert {"k_mix_levels", "k_usb_demod", "k_mix_decimate(level0)", "k_ingest"} <= seen, seen
    for f, dom in (("current_pmc.json", "k_mix_levels"), ("pmc_flat.json", "k_mix_decimate(level0)"), ("pmc_10k.json", "k_mix_levels"),
                   ("pmc_config4.json", "k_mix_levels"), ("pmc_config3_robust.json", "k_mix_levels"), ("pmc_config3_tolerance.json", "k_mix_levels")):
        pm = json.load(open(os.path.join(ROOT, "profiles", f)))
        assert dom in pm["kernels"] and "valu" in pm["kernels"][dom] and "hbm_bytes_per_launch" in pm["kernels"][dom], (f, list(pm["kernels"]))
        assert len({json.load(open(os.path.join(ROOT, "profiles", g)))["build_id"] for g in ("current_pmc.json", f)}) == 1  # one build


def test_printed_line_stays_under_8_kb():
    """the driver could not parse the 22.7 KB line of round 5.  `compact_line` turns everything a run
    measures (here: that very line, committed as profiles/r05/bench_default_with_cpu_baseline.json) into the printed line:
    <= 8 KB, the contract keys, `roofline`, `cpu_baseline`, `verified` and one compact row per side workload."""
    b = _bench()
    full = json.loads([l for l in open(os.path.join(ROOT, "profiles", "r05", "bench_default_with_cpu_baseline.json")) if l.startswith("{")][0])
    assert len(json.dumps(full)) > 20000
    line = b.compact_line(full)
    text = json.dumps(line)
    assert len(text) <= 8192 and json.loads(text) == line
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline", "verified", "build_id"):
        assert k in line, k
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "algorithmic_GBps", "algorithmic_over_hbm_peak",
              "frac_hbm_unique", "pmc_build_id", "pmc_matches_build"):
        assert k in line["roofline"], k
    assert set(line["config"]) >= {"workload", "name", "arithmetic"} and line["verified"]["ok"] is True
    for k in ("north_star_10k", "flat_1024", "config4_256", "fast_config3", "fast_10k", "fast_config4", "config5_64k_one_gpu"):
        row = line[k]
        assert set(row) >= {"ms_per_step", "frame_frac", "bound", "frac", "verified_ok"} and len(json.dumps(row)) < 400, (k, row)
    # a line that would still come out too long loses optional parts, never a contract key
    fat = dict(full, **{k: dict(full["north_star_10k"], workload="x" * 3000) for k in b.SIDE_KEYS})
    fat["config"] = dict(full["config"], workload="y" * 7000)
    slim = b.compact_line(fat)
    assert len(json.dumps(slim)) <= 8192 and "roofline" in slim and "cpu_baseline" in slim and "value" in slim


def test_dump_outputs_writes_what_a_caller_fetches_within_64_mb(tmp_path):
    """`--dump-outputs DIR` (bench.dump_outputs), here over a stand-in receiver: the payloads come from a fetch after the last
    step, one float32 file per publishing leaf -- every leaf of config 3 (31 MB), the seeded sample of the 10 240-sub tree
    whose leaves would not fit -- never more than 64 MB, the same files every time, rank-prefixed at N > 1."""
    import numpy as np
    from sdrreceiver_amd import topology as tp
    b = _bench()

    class Rx:
        def __init__(self, topo):
            self.topo, self.fetched, self.publish = topo, 0, True

        def set_publish(self, on):
            self.publish = on

        def fetch(self):
            assert not self.publish  # (the payloads are read below, not handed to a publish callback per leaf)
            self.fetched += 1

        def output(self, i):
            assert self.fetched, "payloads read before the fetch that completes the last frame"
            v = self.topo.vfos[i]
            n = (v.samples_per_buffer >> v.decimate_count) // (v.late_decimate or 1)
            return ((np.arange(n) * (i + 1)) % 601 - 300).astype(np.int16 if v.demod_usb else np.int8)

    class Job:
        def __init__(self, topo):
            self.topo, self.rx = topo, Rx(topo)

    topo = tp.config3(1024)
    leaves = [i for i in range(len(topo.vfos)) if not topo.children(i)]
    n, nbytes = b.dump_outputs(Job(topo), str(tmp_path / "a"))
    files = sorted(os.listdir(tmp_path / "a"))
    assert n == len(leaves) == len(files) == 1024 and files[0] == f"vfo{leaves[0]:05d}.npy" and nbytes <= b.DUMP_LIMIT
    a = np.load(tmp_path / "a" / files[-1])
    rx = Rx(topo)
    rx.fetched = 1
    assert a.dtype == np.float32 and np.array_equal(a, rx.output(leaves[-1]).astype(np.float32))

    big = tp.config3(10240)
    n, nbytes = b.dump_outputs(Job(big), str(tmp_path / "b"))
    want = tp.sample_leaves(big, 64, b.DUMP_SEED)
    assert n == len(want) and sorted(os.listdir(tmp_path / "b")) == [f"vfo{i:05d}.npy" for i in want] and nbytes <= b.DUMP_LIMIT
    assert b.dump_outputs(Job(big), str(tmp_path / "c")) == (n, nbytes)
    assert all(np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f)) for f in os.listdir(tmp_path / "b"))

    n, nbytes = b.dump_outputs(Job(topo), str(tmp_path / "d"), rank=3, world=4)  # 16 MB per rank: 31 MB of leaves are cut
    assert 0 < n < 1024 and nbytes <= b.DUMP_LIMIT // 4 and all(f.startswith("rank3_vfo") for f in os.listdir(tmp_path / "d"))


DRIVER_COMMAND = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"]
CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                 "data", "config", "build_id")


def _run_bench(cmd):
    """Runs `cmd` in a fresh process: (wall seconds, the one printed line parsed)."""
    import time
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(r.stdout.strip().splitlines()) == 1
    assert len(lines[0]) <= 8192, len(lines[0])
    d = json.loads(lines[0])
    print(f"bench wall {wall:.1f} s, line {len(lines[0])} bytes, legs in bench_full.json")
    for k in CONTRACT_KEYS:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["scaling"] == "weak" and d["data"] == "synthetic" and d["dtype"] == "f32" and "workload" in d["config"]
    assert abs(d["value"] - d["steps"] * 74496000 / (d["ms_per_step"] * d["steps"] * 1e-3) / 1e6) / d["value"] < 0.01
    for path, v in _fracs(d):
        assert v is None or 0.0 <= v <= 1.0, (path, v)
    full = json.load(open(os.path.join(ROOT, "bench_full.json")))
    assert full["value"] == d["value"] and "legs_s" in full
    return wall, d


@pytest.mark.gpu
def test_the_drivers_exact_command_prints_one_parsable_line_in_time():
    """EXACTLY what the driver runs (`python3 bench.py --gpus 1 --steps 20 --warmup 5`), in a fresh process: one `{`-line of at
    most 8 KB that parses and carries every contract field -- and the run does the headline's work only: at most 30 s of wall
    time besides its warm-up and timed steps (start-up, library load and first launches included), 11 repetitions, none of
    what `--full` adds (round 5's command took 64.7 s and printed 22.7 KB, which was not parsed)."""
    wall, d = _run_bench(DRIVER_COMMAND)
    outside = wall - (d["steps"] + d["warmup"]) * d["ms_per_step"] * 1e-3
    assert outside <= 30.0, (wall, d["ms_per_step"], json.load(open(os.path.join(ROOT, "bench_full.json"))).get("legs_s"))
    assert d["repetitions"] == 11
    for k in ("roofline", "cpu_baseline", "verified", "kernels", "through_abi", "north_star_10k"):
        assert k not in d, k


@pytest.mark.gpu
def test_the_full_command_measures_and_verifies_everything_else():
    """The driver's command with `--full`: within 10 minutes, the same parsable line of at most 8 KB with `roofline`,
    `cpu_baseline`, an oracle-verified timed region, the through-the-ABI figures and EVERY side row, each verified."""
    wall, d = _run_bench(DRIVER_COMMAND + ["--full"])
    full = json.load(open(os.path.join(ROOT, "bench_full.json")))
    assert wall <= 600.0, (wall, full.get("legs_s"))
    assert full["repetitions"] == 25
    for k in ("roofline", "cpu_baseline", "verified"):
        assert k in d, k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_GBps"):
        assert k in d["roofline"], k
    # the line says that what it timed is what the oracle computes (bench.Verifier): the launch sequence of the timed region
    ver = d["verified"]
    assert ver["ok"] is True and ver["leaves"] >= 32 and ver["checkpoints"] >= 3 and ver["frames"] >= 3 * 20
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"], k
    assert d["cpu_baseline"]["kind"] in ("reference", "port")
    assert "u8_dc_pipelined_ms" in d["through_abi"]
    # the side rows: every one measured and verified against the oracle
    for k in ("north_star_10k", "fast_config3", "robust_config3", "config4_256", "flat_10k", "fast_10k", "fast_config4", "robust_10k",
              "robust_config4", "flat_1024", "config5_64k_one_gpu"):
        assert d[k].get("verified_ok") is True, (k, d[k])
    # everything else is beside the line
    assert "valu" in full["roofline"] and "through_abi" in full
