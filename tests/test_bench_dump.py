"""bench.py --dump-outputs on the CPU: which arrays of a step are its outputs,
how an output over its share of the budget is sampled (the same rows every
time, in order), the dtypes that keep every value exact, and the files."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

torch = pytest.importorskip("torch")


def test_step_outputs_by_kind():
    inp = {"iv": 1, "oseq": 2, "oflags": 3, "data": 4}
    out = 0
    names = {k: sorted(bench.step_outputs(bench.CONFIGS[k], inp, out))
             for k in ("c2", "c3", "hmac512", "ph_iv", "hmac_verify_mtu",
                       "burst_rx", "burst_tx")}
    assert names == {"c2": ["digests"], "c3": ["digests"], "hmac512": ["digests"],
                     "ph_iv": ["iv"], "hmac_verify_mtu": ["result"],
                     "burst_rx": ["flags", "iv", "result", "seq"],
                     "burst_tx": ["datagrams", "result"]}
    assert bench.step_outputs(bench.CONFIGS["burst_tx"], inp, out)["datagrams"] == 4


def test_sample_outputs_budget_rows_and_dtypes(monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 1 << 16)
    g = torch.Generator().manual_seed(1)
    dig = torch.randint(0, 256, (5003, 32), dtype=torch.uint8, generator=g)
    flat = torch.randint(0, 256, (100_001,), dtype=torch.uint8, generator=g)
    seq = torch.arange(5003, dtype=torch.int32) + (1 << 30)   # past float32's 2^24
    small = torch.randint(0, 256, (7, 1), dtype=torch.uint8, generator=g)
    outs = {"digests": dig, "datagrams": flat, "seq": seq, "result": small}
    a = bench.sample_outputs(outs)
    b = bench.sample_outputs(outs)
    assert sum(v.nbytes for v in a.values()) <= 1 << 16
    for k in outs:
        assert np.array_equal(a[k], b[k])
    share = (1 << 16) // 4
    # a sample of whole rows, in order, drawn from the seed alone
    keep = share // (4 * 32)
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(5003, keep, replace=False))
    assert a["digests"].dtype == np.float32 and a["digests"].shape == (keep, 32)
    assert np.array_equal(a["digests"], dig.numpy()[rows].astype(np.float32))
    # a flat byte buffer: rows of 256 bytes
    assert a["datagrams"].shape == (share // (4 * 256), 256)
    frows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(
        100_001 // 256, share // (4 * 256), replace=False))
    assert np.array_equal(a["datagrams"],
                          flat.numpy()[:100_001 // 256 * 256].reshape(-1, 256)[frows])
    # 32-bit words as float64: exact
    assert a["seq"].dtype == np.float64 and a["seq"].shape == (share // 8,)
    assert set(a["seq"].astype(np.int64)) <= set(seq.numpy().astype(np.int64))
    # under its share: whole
    assert np.array_equal(a["result"], small.numpy().astype(np.float32))
    bench.write_outputs(str(tmp_path / "d"), a)
    bench.write_outputs(str(tmp_path / "d"), {"digests": a["digests"]}, rank=1)
    assert sorted(os.listdir(tmp_path / "d")) == [
        "datagrams.npy", "digests.npy", "digests.rank1.npy", "result.npy", "seq.npy"]
    assert np.array_equal(np.load(tmp_path / "d" / "seq.npy"), a["seq"])
