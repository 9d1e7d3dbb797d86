"""Committed vectors of the oracle's TPFA problem over every combination of graded widths, Dirichlet sides, saturation functions and
completed wells (tests/golden/problem_vectors.npz, made by tests/golden/make_problem_vectors.py from the separate reference classes
that the one ``oracle.tpfa.Problem`` replaced): the one class still reproduces them."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_problem_vectors", os.path.join(HERE, "golden", "make_problem_vectors.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

_file = np.load(os.path.join(HERE, "golden", "problem_vectors.npz"), allow_pickle=False)
GOLD = {k: _file[k] for k in _file.files}
TOL = 1e-9                                  # test_golden_vectors' bound for "same code, round-off only"


def relmax(a, b):
    """Largest difference against the reference's largest magnitude (0 for two all-zero arrays)."""
    d, s = np.abs(a - b).max(), np.abs(b).max()
    return 0.0 if d == 0.0 else d/max(s, 1e-300)


def test_every_case_of_the_fixture_is_computed():
    assert sorted({k.split("/")[0] for k in GOLD}) == sorted(gen.ALL_CASES)


@pytest.mark.parametrize("name", sorted(gen.ALL_CASES))
def test_problem_reproduces_golden_vectors(name):
    out = gen.compute(name)
    assert sorted(out) == sorted(k.split("/", 1)[1] for k in GOLD if k.startswith(name + "/"))
    for k, v in out.items():
        g = GOLD[name + "/" + k]
        assert np.shape(v) == g.shape, k
        if k == "J":                        # per block against the block's own maximum
            b = g.shape[1]
            errs = [relmax(v[:, r, c], g[:, r, c]) for r in range(b) for c in range(b)]
        else:
            errs = [relmax(np.asarray(v), g)]
        print("%s %s: relmax %.3e" % (name, k, max(errs)))
        assert max(errs) < TOL, (k, max(errs))
