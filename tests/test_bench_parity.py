"""bench.py's parity helpers (the `parity` block of the bench line) on fabricated CPU data: a row
counts as matching only when every output is bit-identical -- NaN payloads and signed zeros compared by bits, not by
value -- and a failed fit matches the oracle only with NaN coefficients."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")


@pytest.fixture
def bench():
    # imported inside the tests: bench.py sets GPU_MAX_HW_QUEUES at import, which must not leak into a GPU test run
    # that merely collects this file
    sys.path.insert(0, ROOT)
    import bench as b
    return b


def _outs(n=6, k=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(coef=torch.randn((n, k), generator=g, dtype=torch.float64),
                ll=torch.randn(n, generator=g, dtype=torch.float64),
                status=torch.zeros(n, dtype=torch.int32), n_eval=torch.full((n,), 40, dtype=torch.int32),
                n_grad=torch.full((n,), 5, dtype=torch.int32), flags=torch.zeros(n, dtype=torch.uint8))


def test_outputs_match_is_bitwise(bench):
    a = _outs()
    b = {k: v.clone() for k, v in a.items()}
    assert bench.outputs_match(a, b).all()
    b["coef"][1, 2] = -0.0 if a["coef"][1, 2] == 0.0 else np.nextafter(a["coef"][1, 2].item(), np.inf)
    b["ll"][3] = float("nan")
    a["ll"][4] = float("nan")
    b["ll"][4] = float("nan")                   # same NaN bits: still a match
    b["n_eval"][5] += 1
    m = bench.outputs_match(a, b)
    assert m.tolist() == [True, False, True, False, True, False]


def test_same_bits_distinguishes_signed_zero(bench):
    a = torch.tensor([0.0, 1.0], dtype=torch.float64)
    b = torch.tensor([-0.0, 1.0], dtype=torch.float64)
    assert bench.same_bits(a, b).tolist() == [False, True]


def test_oracle_row_parity_counts_rows(bench):
    n, (p, q, I) = 4, (2, 2, 1)
    rng = np.random.default_rng(1)
    coef = rng.uniform(-0.3, 0.3, size=(n, I + p + q))
    exp = dict(status=np.array([0, 0, 1, 0], dtype=np.int32), n_eval=np.array([30, 31, 10000, 40], dtype=np.int32),
               n_grad=np.array([4, 4, 90, 5], dtype=np.int32), coef=coef.copy(), ll=rng.normal(size=n), pqi=(p, q, I))
    exp["coef"][2] = np.nan
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    flags = np.array([O.model_flags(exp["coef"][i], p, q, I) if exp["status"][i] == 0 else 0 for i in range(n)],
                     dtype=np.uint8)
    res = dict(status=exp["status"].copy(), n_eval=exp["n_eval"].copy(), n_grad=exp["n_grad"].copy(),
               coef=exp["coef"].copy(), ll=exp["ll"].copy(), flags=flags)
    assert bench.oracle_row_parity(res, exp) == n
    res["coef"][0, 0] = np.nextafter(res["coef"][0, 0], np.inf)    # one ulp off: row 0 no longer matches
    res["coef"][2, 1] = 0.0                                          # a failed fit must report NaN coefficients
    res["n_grad"][3] += 1
    assert bench.oracle_row_parity(res, exp) == 1


def test_dump_rows_is_every_row_or_a_fixed_sample_within_the_limit(bench):
    values = 10                                       # C2: 5 coefficients + LL, status, n_eval, n_grad, flags
    cap = bench.DUMP_BYTES // (8 * (values + 1))
    assert bench.DUMP_BYTES <= 64_000_000
    assert np.array_equal(bench.dump_rows(cap, values), np.arange(cap))
    rows = bench.dump_rows(1 << 20, values)
    assert len(rows) == cap < 1 << 20 and len(rows) * 8 * (values + 1) <= bench.DUMP_BYTES
    assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < 1 << 20
    assert np.array_equal(rows, bench.dump_rows(1 << 20, values))      # the same sample in every run
    assert len(bench.dump_rows(1 << 20, values, world=8)) == cap // 8   # the limit holds over all ranks together


def test_dump_outputs_writes_float64_arrays_of_the_first_n_rows(bench, tmp_path):
    outs = _outs(n=7)
    outs["coef"][2, 1] = float("nan")
    bench.dump_outputs(str(tmp_path / "d"), outs, 6, 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(f"{k}.npy" for k in list(outs) + ["rows"])
    assert np.array_equal(np.load(tmp_path / "d" / "rows.npy"), np.arange(6, dtype=np.float64))
    for k, v in outs.items():
        a = np.load(tmp_path / "d" / f"{k}.npy")
        assert a.dtype == np.float64 and a.shape == tuple(v[:6].shape)
        assert np.array_equal(a, v[:6].numpy().astype(np.float64), equal_nan=True)
    bench.dump_outputs(str(tmp_path / "d"), outs, 6, 1, 2)             # several ranks: one set of files per rank
    assert os.path.exists(tmp_path / "d" / "coef.rank1.npy")


def test_dump_outputs_samples_rows_when_the_arrays_exceed_the_limit(bench, tmp_path, monkeypatch):
    n, values = 500, 10
    outs = _outs(n=n + 3)
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 120 * 8 * (values + 1))     # room for 120 rows on each of 2 ranks
    bench.dump_outputs(str(tmp_path), outs, n, 1, 2)
    rows = np.load(tmp_path / "rows.rank1.npy")
    assert rows.dtype == np.float64 and len(rows) == 120 and (np.diff(rows) > 0).all() and rows[-1] < n
    idx = rows.astype(np.int64)
    assert np.array_equal(idx, bench.dump_rows(n, values, 2))
    total = rows.nbytes
    for k, v in outs.items():
        a = np.load(tmp_path / f"{k}.rank1.npy")
        assert a.dtype == np.float64 and np.array_equal(a, v.numpy()[idx].astype(np.float64))
        total += a.nbytes
    assert 2 * total <= bench.DUMP_BYTES
