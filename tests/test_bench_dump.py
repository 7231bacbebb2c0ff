"""bench.py's host-side pieces (no GPU): --dump-outputs' file format and sampling, and what a plain run
(no --full) switches off."""
import os
import sys

import numpy as np

import bench
from nemo_amd.engine import Engine


def _parse(argv):
    old = sys.argv
    sys.argv = ["bench.py"] + argv
    try:
        return bench.parse()
    finally:
        sys.argv = old


def test_plain_run_has_no_side_legs():
    a = _parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 1, False, None)
    assert a.no_cpu_baseline and a.e2e_runs == 0 and a.diff_reps == 0 and a.kernel_timing == "none"


def test_full_keeps_every_leg_and_its_options():
    a = _parse(["--full"])
    assert not a.no_cpu_baseline and a.e2e_runs == 2000 and a.diff_reps == 5 and a.kernel_timing == "dominant"
    a = _parse(["--full", "--no-cpu-baseline", "--e2e-runs", "0", "--kernel-timing", "off"])
    assert a.no_cpu_baseline and a.e2e_runs == 0 and a.kernel_timing == "off"


def _step_results(rng, V=1003, G=6, n_chains=17, F=3, V0=50, R=5, W=2):
    return {"state": rng.integers(0, 256, (V + 3) // 4).astype(np.uint8),
            "chain_off": np.sort(rng.integers(0, n_chains, G + 1)).astype(np.uint64),
            "chain_ht": rng.integers(0, 65536, (n_chains, 2)).astype(np.uint16),
            "masks": rng.integers(0, 2, (F, V0)).astype(np.uint8),
            "missing": rng.integers(0, 2 ** 32, (4, 2), dtype=np.uint64).astype(np.uint32),
            "protos": {"achieved": 4, "inter": [1, 33], "union": [1, 2, 33], "pre_holds": 2 ** 40 + 1, "n_runs": R},
            "tables": rng.integers(0, 2 ** 32, (R, W), dtype=np.uint64).astype(np.uint32),
            "missing_inter": rng.integers(0, 2 ** 32, (F, W), dtype=np.uint64).astype(np.uint32),
            "missing_union": rng.integers(0, 2 ** 32, (F, W), dtype=np.uint64).astype(np.uint32),
            "triggers": (np.arange(6, dtype=np.uint32).reshape(2, 3), np.zeros((0, 2), np.uint32),
                         np.array([9, 4, 7], np.uint32))}


def test_dump_is_exact_and_float(tmp_path):
    V = 1003
    o = _step_results(np.random.default_rng(1), V=V)
    d = str(tmp_path / "out")
    bench.dump_outputs(d, bench.named_outputs(o, V))
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert set(got) == {"node_state", "chain_off", "chain_ht", "missing_events", "diff_masks", "proto_inter",
                        "proto_union", "proto_scalars", "run_tables", "missing_inter", "missing_union",
                        "trigger_pre", "trigger_post", "trigger_async"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    alive, holds = Engine.unpack_state(o["state"], V)
    assert np.array_equal(got["node_state"], alive + 2 * holds)
    assert np.array_equal(got["chain_ht"], o["chain_ht"]) and got["chain_ht"].shape == o["chain_ht"].shape
    assert np.array_equal(got["missing_events"], o["missing"])          # u32 values: exact in float64
    assert got["proto_scalars"].tolist() == [4, 2 ** 40 + 1, 5]
    bits = np.unpackbits(o["tables"].view(np.uint8), axis=1, bitorder="little").reshape(-1)
    assert np.array_equal(got["run_tables"], bits)
    assert got["trigger_async"].tolist() == [4, 7, 9] and got["trigger_post"].size == 0


def test_large_arrays_are_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 2 * 100)  # 100 elements per array
    V = 4001
    rng = np.random.default_rng(2)
    named = {"node_state": (rng.integers(0, 256, (V + 3) // 4).astype(np.uint8), 2, V),
             "small": np.arange(7, dtype=np.uint32)}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, named)
    bench.dump_outputs(b, named)
    s = np.load(os.path.join(a, "node_state.npy"))
    assert s.shape == (100,) and np.array_equal(s, np.load(os.path.join(b, "node_state.npy")))
    assert np.load(os.path.join(a, "small.npy")).tolist() == list(range(7))
    # the sample reads the elements it names: one changed node changes the dump iff it was drawn
    alive, holds = Engine.unpack_state(named["node_state"][0], V)
    full = (alive + 2 * holds).astype(np.float32)
    idx = np.sort(np.random.default_rng([bench.DUMP_SEED, bench.zlib.crc32(b"node_state")]).integers(0, V, 100))
    assert np.array_equal(s, full[idx])
