"""bench.py --dump-outputs on the host: what lands in DIR/<name>.npy (no GPU needed)."""
import os

import numpy as np

import bench


def test_dump_outputs_keeps_float64_and_casts_the_rest_to_float32(tmp_path):
    arrays = {'metrics': np.linspace(0, 1, 8), 'params': np.arange(100, dtype=np.float32).reshape(10, 10),
              'masks': (np.arange(12) % 3 == 0).reshape(3, 4).astype(np.uint8)}
    bench.dump_outputs(str(tmp_path / 'd'), arrays)
    assert sorted(os.listdir(str(tmp_path / 'd'))) == ['masks.npy', 'metrics.npy', 'params.npy']
    for name, want in arrays.items():
        got = np.load(str(tmp_path / 'd' / (name + '.npy')))
        assert got.dtype == (np.float64 if want.dtype == np.float64 else np.float32), name
        assert got.shape == want.shape and np.array_equal(got, want), name       # under the budget: whole, unchanged


def test_dump_outputs_over_the_budget_is_the_same_seeded_sample_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 24000)
    arrays = {'a': np.arange(10000, dtype=np.float32), 'b': -np.arange(1000, dtype=np.float64)}     # 48 000 bytes
    for d in ('one', 'two'):
        bench.dump_outputs(str(tmp_path / d), arrays)
    total = 0
    for name, full in arrays.items():
        one, two = (np.load(str(tmp_path / d / (name + '.npy'))) for d in ('one', 'two'))
        assert np.array_equal(one, two), name                        # fixed positions: two builds compare element for element
        assert one.dtype == full.dtype and 0 < one.size < full.size, name
        assert np.all(np.isin(one, full)) and np.all(np.diff(np.abs(one)) > 0), name      # distinct elements, in order
        total += one.nbytes
    assert total <= 24000
