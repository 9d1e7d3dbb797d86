"""The Jacobi sweeps' centre-cell omega / diag recomputed in registers (k_amg_jacobi, k_amg_prolong_jacobi, k_amg_prolong2_jacobi;
DESIGN.md 4.5) against the plane k_amg_weights stored, which TP_AMG_INVD_LOAD=1 keeps reading: the same correctly rounded
division and the same rounding to the storage type, so every comparison is BITWISE.

The switch is read once per process: tests/invd_env_check.py runs every case in one child process per setting, once for the
whole module, and the tests compare the arrays the two children wrote."""
import numpy as np
import pytest

from switches import run_children

pytestmark = pytest.mark.gpu

SETTINGS = {"registers": {}, "load": {"TP_AMG_INVD_LOAD": "1"}}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return run_children("invd_env_check.py", SETTINGS, tmp_path_factory.mktemp("invd"), timeout=600)         # the children side by side


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_pc_apply_bitwise(runs):
    """One pc_apply on the 30 x 110 x 40 box, registers against the stored plane."""
    y = runs["registers"]["pc_apply_30x110x40"]
    assert np.isfinite(y).all() and np.abs(y).max() > 0
    assert same_bits(y, runs["load"]["pc_apply_30x110x40"])


@pytest.mark.parametrize("case", ["unfused_13x11x9", "fp32_operators", "gs_levels", "line_levels", "truncated", "slabs2_8x21x7"])
def test_vcycles_bitwise(runs, case):
    """V-cycles on the unfused path, with fp32 operators, next to Gauss-Seidel, line and truncation levels (which keep the
    stored plane), and on two slabs."""
    reg, load = runs["registers"], runs["load"]
    if case == "truncated":
        assert tuple(reg[case + "_trunc"]) == (0, 0)
    if case == "slabs2_8x21x7":
        assert reg[case + "_dist"][0] >= 1             # distributed top levels
    keys = [k for k in (case + "_v0", case + "_v1") if k in reg]
    assert keys
    for k in keys:
        assert np.isfinite(reg[k]).all() and np.abs(reg[k]).max() > 0, k
        assert same_bits(reg[k], load[k]), k
