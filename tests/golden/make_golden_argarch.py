"""Writes tests/golden/argarch/*.npz: the ARGARCH fit fixtures (inputs and the results the pure-Python restatement
tests/argarch_ref.py records for them). Run from the repository root: python tests/golden/make_golden_argarch.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import argarch_ref as R  # noqa: E402


def main():
    os.makedirs(os.path.join(HERE, "argarch"), exist_ok=True)     # a folder of their own: the ARIMA suites glob golden/*.npz
    for name in R.FIXTURES:
        rows = R.fixture_rows(name)
        f = R.fit_batch(rows)
        meta = dict(name=name, model="argarch", N=int(rows.shape[0]), T=int(rows.shape[1]))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), meta=json.dumps(meta), series=rows, coef=f["coef"],
                            obj=f["obj"], status=f["status"], n_eval=f["n_eval"], n_grad=f["n_grad"],
                            ar_status=f["ar_status"])
        print(name, "AR", np.bincount(f["ar_status"]).tolist(), "fit", np.bincount(f["status"]).tolist(),
              int(f["n_eval"].max()))


if __name__ == "__main__":
    main()
