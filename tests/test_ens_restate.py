"""The restatement of the ensemble consensus stage (tests/ens_restate.py) against the reference's stored results
(tests/golden/ens_*.npz): it is the oracle of the GPU tests at the edges of the launch geometry, so it is held to the
reference first.  No GPU needed (the consensus rows go through the library's host-only greedy union)."""
import glob
import os

import numpy as np
import pytest

import ens_restate as er
from util import GOLDEN

CASES = sorted(os.path.basename(f)[4:-4] for f in glob.glob(os.path.join(GOLDEN, "ens_*.npz")))


def test_all_cases_are_here():
    assert len(CASES) == 11, CASES


@pytest.mark.parametrize("name", CASES)
def test_restatement_against_golden(name):
    z = np.load(os.path.join(GOLDEN, "ens_%s.npz" % name))
    seqs = [str(s) for s in z["seqs"]]
    members = [["".join(r) for r in m] for m in z["members"]]
    t = er.Table.of_members(members, [len(s) for s in seqs])
    assert t.runs == len(members)
    for k, rows in enumerate(members):
        assert t.score(rows)[1] == pytest.approx(float(z["scores"][k]), rel=1e-9, abs=1e-9), k
    r, c = t.confidence(members[0])
    assert np.array_equal(r, z["m0_res_conf"]) and np.array_equal(c, z["m0_col_conf"])
    for m in (int(x) for x in z["min_supports"]):
        rows = [x.decode() for x in t.consensus(seqs, m)]
        assert rows == [str(x) for x in z["cons%d" % m]], m
        assert t.score(rows)[1] == pytest.approx(float(z["cons%d_score" % m]), rel=1e-9, abs=1e-9), m
        r, c = t.confidence(rows)
        assert np.array_equal(r, z["cons%d_res_conf" % m]), m
        assert np.array_equal(c, z["cons%d_col_conf" % m]), m
