"""The default path of the composite preconditioner before and after pc_order: this script runs the default
order -- no pc_order key anywhere -- on the parity systems of tests/pc_order_ref.py and on one Newton solve, and writes every
output to the .npz path given as argv[1].  argv[2], if given, is the root of ANOTHER checkout of this repository (one of the
parent commit, built) whose package is imported instead of this one: the two .npz files must hold identical arrays
(profiles/pc_order_parity.txt is that comparison, made by running this script once per checkout and `compare` below).

    python tests/pc_order_env_check.py new.npz
    python tests/pc_order_env_check.py old.npz /path/to/parent/checkout
    python tests/pc_order_env_check.py --compare old.npz new.npz"""
import os
import sys

import numpy as np

from switches import ROOT, child_main


def main(root=ROOT):
    sys.path.insert(0, root)                                 # in front of this checkout's root; cases.py and pc_order_ref.py
    import cases                                             # stay those of THIS checkout (inputs only)
    import pc_order_ref as PR
    from thermalporous_amd import engine as E
    assert os.path.dirname(os.path.dirname(os.path.abspath(E.__file__))) == os.path.abspath(root), E.__file__
    out = {}
    for name, builder, kw, opts in PR.PARITY:
        spec, u0, *_ = getattr(cases, builder)(**kw)
        u = cases.perturbed_state(spec, seed=5, amp=0.3)
        h = E.HipEngine(spec, opts)
        h.set_old(u0)
        h.set_dt(PR.DT)
        h.set_state(u)
        h.jacobian()
        h.pc_setup()
        h.vec_set("x", np.random.default_rng(11).standard_normal(u.shape))
        h.pc_apply("x", "y")
        out[name + ".pc_apply"] = h.vec_get("y")
        h.stage1_apply("x", "y")
        out[name + ".stage1"] = h.vec_get("y")
        h.residual()
        h.copy_residual_to("b")
        its, reason, rn = h.fgmres("b", "d")
        out[name + ".fgmres"] = h.vec_get("d")
        out[name + ".fgmres_counts"] = np.array([its, reason, rn])
        h.close()
    spec, u0, *_ = cases.c4_spe10_3d(Nx=7, Ny=13, Nz=9, nphase=2)
    h = E.HipEngine(spec, dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25))
    h.set_state(u0)
    h.set_old(u0)
    h.set_dt(86.4)
    r = h.newton_solve()
    out["newton.counts"] = np.array([r["nits"], r["lits"], r["reason"], r["vcycles"]])
    out["newton.fnorm"] = np.array(r["fnorm"])
    out["newton.x"] = h.get_state()
    h.close()
    return out


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), (A.files, B.files)
    same = True
    for k in sorted(A.files):
        eq = A[k].shape == B[k].shape and np.array_equal(A[k], B[k])
        same = same and eq
        print("%-34s %-16s %s" % (k, A[k].shape, "identical" if eq else "DIFFERENT (max |a - b| = %.3e)" % np.abs(A[k] - B[k]).max()))
    print("all identical" if same else "NOT identical")
    return 0 if same else 1


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    child_main(lambda: main(*sys.argv[2:3]))
