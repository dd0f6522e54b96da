#!/usr/bin/env python3
"""Generate tests/golden/clinical_tests.json by RUNNING THE REFERENCE's own four clinical-variable tests
(``pilotpy/tools/Trajectory.py``: correlation_categorical_with_trajectory, correlation_numeric_with_trajectory,
correlation_categorical_with_clustering, correlation_numeric_with_clustering) on a seeded synthetic cohort.

Runs only where the reference is present (``gen_golden.import_reference``); the tests read the committed file.  The file holds
data only: the inputs (``obs``, ``orders``, ``proportion_df`` as column -> list, a missing value as null) and, per function, the
feature list it was called with and the frame it returned (columns, index, rows).  Floats are written with ``repr`` precision,
so they read back to the same bits.

The cohort: 36 samples, two cells each (the second cell of a sample carries ANOTHER value of ``sex``: only a sample's first
occurrence counts).  ``sex`` and ``age`` follow the pseudotime, ``stage`` follows the sub-groups, ``centre`` and ``bmi`` are noise
(they fail the 0.05 filter), ``egfr`` has a missing value, and ``grade`` mixes numeric strings with labels and a missing value.
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

from gen_golden import import_reference  # noqa: E402

OUT = os.path.join(HERE, "clinical_tests.json")
CATEGORICAL = ["sex", "centre", "stage", "grade"]
NUMERIC = ["age", "bmi", "egfr"]


def cohort(seed=20261021, n=36):
    rs = np.random.RandomState(seed)
    samples = ["P%02d" % i for i in range(n)]
    time = np.round(rs.permutation(n) / float(n - 1), 6)
    labels = np.array([str(v) for v in (time * 2.999).astype(int)], dtype=object)
    labels[rs.choice(n, 6, replace=False)] = "1"
    sex = np.where(time + 0.35 * rs.randn(n) > 0.5, "M", "F").astype(object)
    centre = rs.choice(["north", "south", "west"], n).astype(object)
    stage = np.array(["early", "mid", "late"], dtype=object)[np.clip(labels.astype(int) + (rs.rand(n) < 0.15), 0, 2)]
    age = np.round(40 + 30 * time + 6 * rs.randn(n), 1)
    bmi = np.round(25 + 3 * rs.randn(n), 1)
    egfr = np.round(90 - 40 * time + 8 * rs.randn(n), 1)
    egfr[7] = np.nan
    grade = np.array([str(v) for v in rs.randint(1, 4, n)], dtype=object)
    grade[time > 0.7] = "high"
    grade[time < 0.2] = "low"
    grade[11] = np.nan
    rows = []
    for i in range(n):
        for cell in range(2):
            rows.append({"sampleID": samples[i], "sex": sex[i] if cell == 0 else ("F" if sex[i] == "M" else "M"), "centre": centre[i],
                         "stage": stage[i], "age": age[i], "bmi": bmi[i], "egfr": egfr[i], "grade": grade[i]})
    obs = pd.DataFrame(rows)
    shuffled = rs.permutation(n)
    orders = pd.DataFrame({"sampleID": [samples[i] for i in shuffled], "Time_score": time[shuffled]})
    proportion_df = pd.DataFrame({"ct0": np.round(rs.rand(n), 4), "Predicted_Labels": labels, "sampleID": samples})
    return obs, orders, proportion_df


def columns_of(frame):
    out = {}
    for c in frame.columns:
        out[c] = [None if (isinstance(v, float) and v != v) else (v.item() if isinstance(v, np.generic) else v) for v in frame[c].tolist()]
    return out


def frame_record(frame):
    return {"columns": list(frame.columns), "index": [int(i) for i in frame.index], "data": columns_of(frame)}


def main():
    T = import_reference()
    obs, orders, proportion_df = cohort()
    adata = types.SimpleNamespace(obs=obs, uns={"orders": orders})
    calls = {
        "correlation_categorical_with_trajectory": (lambda f: T.correlation_categorical_with_trajectory(adata, features=f), CATEGORICAL),
        "correlation_numeric_with_trajectory": (lambda f: T.correlation_numeric_with_trajectory(adata, features=f), NUMERIC),
        "correlation_categorical_with_clustering": (lambda f: T.correlation_categorical_with_clustering(adata, proportion_df, features=f),
                                                    CATEGORICAL),
        "correlation_numeric_with_clustering": (lambda f: T.correlation_numeric_with_clustering(adata, proportion_df, features=f), NUMERIC),
    }
    record = {"obs": columns_of(obs), "orders": columns_of(orders), "proportion_df": columns_of(proportion_df), "results": {}}
    for name, (call, features) in calls.items():
        frame = call(list(features))
        print(name, "kept", list(frame["Feature"]), "of", features)
        print(frame)
        record["results"][name] = {"features": list(features), "frame": frame_record(frame)}
    with open(OUT, "w") as f:
        json.dump(record, f, indent=1, allow_nan=False)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
