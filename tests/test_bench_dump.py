"""bench.py --dump-outputs: the arrays of the last timed step as float32 / float64 .npy files within 64 MB, the clip-token rows a fixed
seeded sample, one set per rank at N > 1.  CPU-only: the writer on host tensors of the bench's shapes."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_files_dtypes_and_budget(tmp_path):
    b = _bench()
    ids = torch.randint(0, 50272, (32, 32), dtype=torch.int64)
    feats = torch.randn(32 * 17 * 32, 2560).to(torch.bfloat16)  # the default step's projected clip tokens
    for run in ("a", "b"):
        b.dump_outputs(str(tmp_path / run), ids, feats, 0, 1)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["clip_tokens_sample.npy", "clip_tokens_sample_rows.npy", "generated_ids.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    got = {n: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["generated_ids.npy"], ids.numpy()) and got["generated_ids.npy"].dtype == np.float64
    rows = got["clip_tokens_sample_rows.npy"].astype(np.int64)
    assert len(rows) > 1000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["clip_tokens_sample.npy"], feats[torch.from_numpy(rows)].float().numpy())
    for n in names:  # the same rows in every run
        assert np.array_equal(got[n], np.load(tmp_path / "b" / n))


def test_dump_outputs_per_rank_within_one_budget(tmp_path):
    b = _bench()
    ids = torch.zeros((2, 32), dtype=torch.int64)
    feats = torch.randn(32 * 17 * 32, 2560).to(torch.bfloat16)
    for r in range(8):
        b.dump_outputs(str(tmp_path), ids, feats, r, 8)
    names = os.listdir(tmp_path)
    assert sorted(names) == sorted(f"{n}_rank{r}.npy" for n in ("generated_ids", "clip_tokens_sample", "clip_tokens_sample_rows") for r in range(8))
    assert sum(os.path.getsize(tmp_path / n) for n in names) <= 64 << 20
