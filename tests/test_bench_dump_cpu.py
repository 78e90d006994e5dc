"""bench.py --dump-outputs, without a GPU: dump_outputs writes the output ciphertexts exactly (float64), their decryptions
(float32) and the rows written; above the byte budget a fixed sample of rows, the same on every call; --steps below 1 is
refused before anything starts."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_dump_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def key(built_lib):
    import eoc_tfhe_amd as eoc
    return eoc.SecretKey(eoc.default_params(0), 1, with_cloud_key=False)


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("ciphertexts", "bits", "rows")}


def test_whole_output_is_written_exactly(bench, key, tmp_path):
    bits = np.random.default_rng(3).integers(0, 2, 300).astype(np.uint8)
    cts = key.encrypt_bits(bits, 2, 0)
    info = bench.dump_outputs(str(tmp_path / "out"), cts, key)
    assert info["rows"] == info["of"] == 300
    a = _load(tmp_path / "out")
    assert a["ciphertexts"].dtype == np.float64 and a["bits"].dtype == np.float32 and a["rows"].dtype == np.float64
    assert np.array_equal(a["ciphertexts"].astype(np.int32), cts) and np.array_equal(a["ciphertexts"], cts)
    assert np.array_equal(a["bits"], bits) and np.array_equal(a["rows"], np.arange(300))


def test_circuit_planes_are_flattened_to_rows(bench, key, tmp_path):
    bits = np.random.default_rng(4).integers(0, 2, 9 * 16).astype(np.uint8)
    cts = key.encrypt_bits(bits, 5, 0).reshape(9, 16, -1)               # (wires, instances, n + 1)
    bench.dump_outputs(str(tmp_path), cts, key)
    a = _load(tmp_path)
    assert a["ciphertexts"].shape == (9 * 16, cts.shape[-1]) and np.array_equal(a["bits"], bits)


def test_large_output_is_a_fixed_sample_within_the_budget(bench, key, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    bits = np.random.default_rng(5).integers(0, 2, 2000).astype(np.uint8)
    cts = key.encrypt_bits(bits, 7, 0)                                  # 2000 rows x 501 x 8 B: about 8 MB in float64
    bench.dump_outputs(str(tmp_path / "a"), cts, key)
    bench.dump_outputs(str(tmp_path / "b"), cts, key)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in a) <= (1 << 20) + 3 * 128   # + the .npy headers
    rows = a["rows"].astype(np.int64)
    assert 0 < rows.size < 2000 and np.all(np.diff(rows) > 0) and rows[-1] < 2000
    assert all(np.array_equal(a[n], b[n]) for n in a)
    assert np.array_equal(a["ciphertexts"], cts[rows]) and np.array_equal(a["bits"], bits[rows])


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr
