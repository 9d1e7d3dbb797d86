"""The opt-in backtracking line search on the GPU (tp_options.ls_kind = 1) against the numpy reference tests/newton_ls_ref.py,
which runs the same algorithm on the oracle's residual, Jacobian and linear solve.

Tolerance of the history comparison (accepted lambdas and ||F|| per Newton iteration): not fixed by hand.  On the CPU the
reference runs every input of newton_ls_ref.PARITY twice, the second time with every linear system solved to ksp_rtol/100 -- two
legitimate Newton directions; the largest relative change of an accepted lambda or a history ||F|| is the floor (2.874e-5, input
B; A: 1.3e-7).  The GPU's Krylov solve differs from the oracle's by its summation order and +-1 iteration, so 10 x the floor is
allowed: newton_ls_ref.PARITY_TOL = 2.9e-4 (profiles/newton_ls_parity.txt; tests/test_newton_ls_host.py re-measures the floor and
checks that every Armijo decision of these inputs lies at least 1e-3 from its threshold, so the decisions themselves -- reason,
iterations, trials per iteration -- must be EQUAL).  States: the tolerance of tests/test_gpu_parity.py's Newton tests, 1e-8.
Inputs A and B are the replaced ones described in newton_ls_ref.py.  The two-slab run uses input B: A's grid is one plane thick
and cannot be cut into slabs."""
import ctypes as C
import threading

import numpy as np
import pytest

import cases
import newton_ls_ref as R

pytestmark = pytest.mark.gpu

_REF = {}
DAY = 86400.0


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def reference(name):
    """(spec, u0, reference result) of a named input, computed once and shared (never modified)."""
    if name not in _REF:
        if name == "D":
            spec, u0, first, d = R.run_ref_D(3)
            _REF[name] = (spec, u0, d)
        elif name == "E":
            _REF[name] = R.run_ref("c3", R.A_OPTS, 0.1, dict(ls_max_it=1))
        elif name == "F":
            _REF[name] = R.run_ref("c3", R.F_OPTS, 0.1, dict(ls_max_change=R.F_CAP))
        else:
            _, case, opts, dt, ls = [p for p in R.PARITY + [R.C_INPUT] if p[0] == name][0]
            _REF[name] = R.run_ref(case, opts, dt, ls)
    return _REF[name]


def gpu_engine(spec, u0, opts, dt_days, **kw):
    from thermalporous_amd.engine import HipEngine
    h = HipEngine(spec, opts, **kw)
    h.set_state(u0)
    h.set_old(u0)
    h.set_dt(dt_days*DAY)
    return h


def check_history(h, info, ref, tag):
    hist = h.ls_history()
    li = h.ls_info()
    dl = max([abs(a - b)/abs(b) for a, b in zip(hist["lam"], ref["lam"])] or [0.0])
    dh = max([abs(a - b)/abs(b) for a, b in zip(hist["fnorm"], ref["hist"])] or [0.0])
    print(tag, "reason", info["reason"], "nits", info["nits"], "lits", info["lits"], "(ref %d)" % ref["lits"], "trials", hist["trials"],
          "evaluations", li["evaluations"], "nonfinite", li["nonfinite"], "max dev lambda %.3e ||F|| %.3e" % (dl, dh))
    print(tag, "lambda", list(hist["lam"]))
    assert info["reason"] == ref["reason"] and info["nits"] == ref["nits"] == hist["n"], (info, ref["reason"], ref["nits"])
    assert hist["trials"] == ref["trials"], (hist["trials"], ref["trials"])
    assert li["kind"] == 1 and li["evaluations"] == ref["evaluations"] == info["ls_trials"] and li["nonfinite"] == len(ref["nonfinite"])
    assert dl <= R.PARITY_TOL and dh <= R.PARITY_TOL, (dl, dh)
    return hist


def check_state(uh, uo):
    assert rel2(uh[0], uo[0]) < 1e-8 and rel2(uh[1], uo[1]) < 1e-8
    if uh.shape[0] == 3:
        assert np.abs(uh[2] - uo[2]).max() < 1e-8


# ---- the two kernels alone ---------------------------------------------------------------------------------------------------------
# internal extents (n0, n1, n2): 2x3x5 (plane of 6 entries: the 16-byte path), 5x7x9 (odd plane: the 8-byte path), 12x16x1 (one
# plane) and 9x11x13 (1287 cells: two blocks of the statistics kernel, a last block that is partly empty in both kernels)
GRIDS = [("5x3x2", cases.c4_spe10_3d, dict(Nx=5, Ny=3, Nz=2)), ("7x9x5", cases.c4_spe10_3d, dict(Nx=9, Ny=5, Nz=7)),
         ("12x16x1", cases.c3_spe10_2d, dict(Nx=12, Ny=16)), ("13x11x9", cases.c4_spe10_3d, dict(Nx=13, Ny=11, Nz=9))]
LAMBDAS = (1.0, 0.5, 0.0625, 0.3, 0.19635756890789216, 1e-3)


def _raw_set(h, name, arr):
    a = np.ascontiguousarray(arr, dtype=float).reshape(-1)
    h._ck(h.lib.tp_vec_set(h.ctx, h.vec(name), a.ctypes.data_as(C.POINTER(C.c_double))))


def _raw_get(h, name):
    out = np.empty(h.b*h.ntot)
    h._ck(h.lib.tp_vec_get(h.ctx, h.vec(name), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out.reshape(h.b, h.n[2] + 2, h.n[1], h.n[0])


def _kernel_checks(h, seed, allreduced=None):
    """Statistics and trial kernels on engine h with seeded vectors whose halo planes hold (finite) random numbers.  Returns the
    owned dx and the statistics; allreduced: the global (sum of squares, maxima) to compare with instead of this slab's."""
    rng = np.random.default_rng(seed)
    sh = (h.b, h.n[2] + 2, h.n[1], h.n[0])
    scale = np.array([50.0, 20.0, 0.03][:h.b]).reshape(-1, 1, 1, 1)
    dx = scale*rng.standard_normal(sh)
    u0 = np.array([41.0, 320.0, 0.9][:h.b]).reshape(-1, 1, 1, 1) + rng.standard_normal(sh)
    junk = rng.standard_normal(sh)
    _raw_set(h, "dx", dx)
    _raw_set(h, "u0", u0)
    own = dx[:, 1:-1]
    ssq, mx = h.ls_step_stats("dx")
    want_ssq, want_mx = (float(np.sum(own*own)), np.abs(own).reshape(h.b, -1).max(axis=1)) if allreduced is None else allreduced
    assert np.array_equal(mx, want_mx), (mx, want_mx)                     # maxima: bitwise
    assert abs(ssq - want_ssq) <= 1e-13*want_ssq, (ssq, want_ssq)
    for lam in LAMBDAS:
        _raw_set(h, "out", junk)
        h.ls_trial("u0", "dx", lam, "out")
        got = _raw_get(h, "out")
        want = u0[:, 1:-1] - lam*dx[:, 1:-1]
        assert np.array_equal(got[:, 0], junk[:, 0]) and np.array_equal(got[:, -1], junk[:, -1]), lam      # halo planes untouched
        if lam in (1.0, 0.5, 0.0625):
            assert np.array_equal(got[:, 1:-1], want), lam                 # lam*dx is exact: fused or not, the same bits
        else:
            # one rounding (the compiler contracts the update into an FMA) against numpy's two: with e the exact value,
            # |want - e| <= ulp(lam dx)/2 + ulp(want)/2 and |got - e| <= ulp(got)/2 -- one ulp of the result plus half an ulp
            # of the product, which is the larger of the two where u0 and lam dx cancel (1.5: got may lie in the next binade)
            prod = lam*dx[:, 1:-1]
            assert np.all(np.abs(got[:, 1:-1] - want) <= 1.5*np.spacing(np.abs(want)) + 0.5*np.spacing(np.abs(prod))), lam
    # in place (out = u0) is allowed: the kernel is elementwise
    h.ls_trial("u0", "dx", 0.5, "u0")
    assert np.array_equal(_raw_get(h, "u0")[:, 1:-1], u0[:, 1:-1] - 0.5*dx[:, 1:-1])
    return own, float(np.sum(own*own))


@pytest.mark.parametrize("nphase", [1, 2])
@pytest.mark.parametrize("name,builder,kw", GRIDS, ids=[g[0] for g in GRIDS])
def test_kernels_alone(name, builder, kw, nphase):
    from thermalporous_amd.engine import HipEngine
    spec, u0, *_ = builder(nphase=nphase, **kw)
    h = HipEngine(spec, dict(pc="cpr"))
    _kernel_checks(h, seed=11 + nphase)
    assert h.ls_info() == dict(kind=0, bytes=0, evaluations=0, nonfinite=0)
    h.close()


@pytest.mark.parametrize("nphase", [1, 2])
def test_kernels_on_two_slabs_with_a_ragged_split(nphase):
    """5x7x9 on two in-process slabs (5 + 4 planes): sums and maxima are all-reduced, every slab updates its own cells."""
    from thermalporous_amd import engine as E
    spec, u0, *_ = cases.c4_spe10_3d(Nx=9, Ny=5, Nz=7, nphase=nphase)
    assert tuple(spec["n"]) == (7, 5, 9)
    lib = E.load_library()
    nslabs = 2
    # the global statistics from the same seeded per-slab vectors (seed = 30 + rank)
    parts = []
    for rank in range(nslabs):
        lo, hi = E.slab_range(9, rank, nslabs)
        rng = np.random.default_rng(30 + rank)
        sh = (nphase + 1, hi - lo + 2, 5, 7)
        dx = np.array([50.0, 20.0, 0.03][:nphase + 1]).reshape(-1, 1, 1, 1)*rng.standard_normal(sh)
        parts.append(dx[:, 1:-1])
    assert [p.shape[1] for p in parts] == [5, 4]
    ssq = float(sum(np.sum(p*p) for p in parts))
    mx = np.max([np.abs(p).reshape(nphase + 1, -1).max(axis=1) for p in parts], axis=0)
    group = C.c_void_p()
    assert lib.tp_local_group_create(nslabs, C.byref(group)) == 0
    err = []

    def worker(rank):
        try:
            h = E.HipEngine(spec, dict(pc="cpr"), rank=rank, nranks=nslabs, local_group=group)
            _kernel_checks(h, seed=30 + rank, allreduced=(ssq, mx))
            h.close()
        except Exception as e:      # noqa: BLE001
            err.append((rank, repr(e)))
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(nslabs)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "slab worker hung"
    lib.tp_local_group_destroy(group)
    assert not err, err


# ---- the search inside tp_newton_solve ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case,opts,dt,ls", R.PARITY, ids=[p[0] for p in R.PARITY])
def test_history_parity(name, case, opts, dt, ls):
    spec, u0, ref = reference(name)
    (reason, nits, trials), (breason, bnits) = R.EXPECT[name]
    assert (ref["reason"], ref["nits"], ref["trials"]) == (reason, nits, trials)
    h = gpu_engine(spec, u0, {**opts, "linesearch": "bt", **ls}, dt)
    info = h.newton_solve()
    check_history(h, info, ref, name)
    check_state(h.get_state(), ref["u"])
    assert info["fnorm"] <= opts.get("snes_rtol", 1e-8)*info["fnorm0"]
    assert h.ls_info()["bytes"] == 8*h.b*h.ntot
    # the same context under basic from the same cold state: the failure the search is there to prevent
    h.set_options(linesearch="basic", ls_order=3)
    h.set_state(u0)
    h.set_old(u0)
    binfo = h.newton_solve()
    print(name, "basic", binfo["reason"], binfo["nits"])
    assert binfo["reason"] < 0
    assert h.ls_history()["n"] == 0 and h.ls_info() == dict(kind=0, bytes=0, evaluations=0, nonfinite=0)
    h.close()


def test_full_steps_are_bitwise_the_basic_solver():
    """Input C: every first trial is accepted; the bt state is the basic state, bit for bit."""
    name, case, opts, dt, ls = R.C_INPUT
    spec, u0, ref = reference("C")
    hb = gpu_engine(spec, u0, opts, dt)
    ib = hb.newton_solve()
    assert ib["reason"] == 3 and ib["ls_trials"] == 0
    assert hb.ls_history()["n"] == 0 and hb.ls_info() == dict(kind=0, bytes=0, evaluations=0, nonfinite=0)       # default untouched
    h = gpu_engine(spec, u0, {**opts, "linesearch": "bt"}, dt)
    info = h.newton_solve()
    hist = h.ls_history()
    assert (info["reason"], info["nits"], info["lits"]) == (ib["reason"], ib["nits"], ib["lits"]) and info["nits"] == ref["nits"]
    assert hist["trials"] == [1]*info["nits"] and list(hist["lam"]) == [1.0]*info["nits"] and info["ls_trials"] == info["nits"]
    assert np.array_equal(h.get_state(), hb.get_state())
    assert info["fnorm"] == ib["fnorm"]
    h.close()
    hb.close()


def test_nonfinite_trials_and_nothing_nonfinite_survives():
    """Input D: lambda = 0.5 and 0.0625 exactly after 1 + 4 non-finite trials; then the same context, switched back to basic,
    reproduces a fresh context bit for bit."""
    spec, u0, ref = reference("D")
    for k, v in R.D_EXPECT.items():
        assert ref[k] == v
    h = gpu_engine(spec, u0, {**R.A_OPTS, "snes_max_it": 1}, R.D_DT)
    first = h.newton_solve()
    assert first["reason"] == -5 and first["nits"] == 1 and np.isfinite(h.get_state()).all()
    h.set_options(linesearch="bt", snes_max_it=2)
    info = h.newton_solve()
    hist, li = h.ls_history(), h.ls_info()
    print("D", info, list(hist["lam"]), hist["trials"], li)
    assert info["reason"] == -5 and info["nits"] == 2
    assert list(hist["lam"]) == [0.5, 0.0625] and hist["trials"] == [2, 5]
    assert li["evaluations"] == 7 and li["nonfinite"] == 5
    assert np.isfinite(h.get_state()).all() and np.isfinite(hist["fnorm"]).all()
    # restore, switch to basic at a small time step, solve: as a context that never saw a non-finite number
    small = dict(R.A_OPTS, snes_max_it=25)
    h.set_options(linesearch="basic", snes_max_it=25)
    h.set_state(u0)
    h.set_old(u0)
    h.set_dt(0.001*DAY)
    again = h.newton_solve()
    fresh = gpu_engine(spec, u0, small, 0.001)
    want = fresh.newton_solve()
    assert again["reason"] == want["reason"] > 0 and (again["nits"], again["lits"]) == (want["nits"], want["lits"])
    assert again["fnorm"] == want["fnorm"] and np.array_equal(h.get_state(), fresh.get_state())
    h.close()
    fresh.close()


def test_failed_search_restores_the_state_bitwise():
    """Input E: ls_max_it 1 on A: reason -6, no iteration, the state is the start state."""
    spec, u0, ref = reference("E")
    assert ref["reason"] == -6
    h = gpu_engine(spec, u0, {**R.A_OPTS, "linesearch": "bt", "ls_max_it": 1}, 0.1)
    info = h.newton_solve()
    assert info["reason"] == -6 and info["nits"] == 0 and info["fnorm"] == info["fnorm0"] and info["ls_trials"] == 1
    assert h.ls_history()["n"] == 0
    assert np.array_equal(h.get_state(), np.asarray(u0).reshape(h.get_state().shape))
    # the context goes on: more trials allowed, the same solve converges as input A does
    h.set_options(ls_max_it=40)
    info = h.newton_solve()
    check_history(h, info, reference("A_order3")[2], "E->A")
    h.close()


def test_first_trial_rule():
    """Input F: the cap on the change of S_o shortens the first trial.  The expected length comes from the GPU's own first
    correction (the Krylov solve newton_solve repeats), with numpy's maximum: 1e-12; the history against the reference's."""
    spec, u0, ref = reference("F")
    assert (ref["reason"], ref["nits"], ref["trials"]) == R.F_EXPECT
    opts = {**R.F_OPTS, "linesearch": "bt", "ls_max_change": R.F_CAP}
    h = gpu_engine(spec, u0, opts, 0.1)
    h.jacobian()
    h.pc_setup()
    h.copy_residual_to("b")
    its, reason, rn = h.fgmres("b", "d")
    assert reason > 0
    dx = h.vec_get("d")
    ssq, mx = h.ls_step_stats("d")
    assert np.array_equal(mx, np.abs(dx).reshape(3, -1).max(axis=1))
    want = min(1.0, R.F_CAP[2]/float(np.abs(dx[2]).max()))
    info = h.newton_solve()
    hist = check_history(h, info, ref, "F")
    assert hist["trials"][0] == 1 and abs(hist["lam"][0] - want) <= 1e-12*want, (hist["lam"][0], want)
    assert abs(hist["lam"][0] - ref["first"][0]) <= R.PARITY_TOL*ref["first"][0]
    check_state(h.get_state(), ref["u"])
    h.close()


def test_two_slabs_agree_with_one():
    """Input B on two in-process slabs: every rank takes the same decisions, and the history is the one-slab history within
    the tolerance (the per-slab stage-2 blocks make it another legitimate Newton direction)."""
    from thermalporous_amd import engine as E
    name, case, opts, dt, ls = [p for p in R.PARITY if p[0] == "B"][0]
    spec, u0, ref = reference("B")
    full = {**opts, "linesearch": "bt", **ls}
    lib = E.load_library()
    nslabs = 2
    group = C.c_void_p()
    assert lib.tp_local_group_create(nslabs, C.byref(group)) == 0
    out, err = [None]*nslabs, []

    def worker(rank):
        try:
            h = gpu_engine(spec, u0, full, dt, rank=rank, nranks=nslabs, local_group=group)
            info = h.newton_solve()
            out[rank] = (info, h.ls_history(), h.ls_info(), h.get_state())
            h.close()
        except Exception as e:      # noqa: BLE001
            err.append((rank, repr(e)))
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(nslabs)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts), "slab worker hung"
    lib.tp_local_group_destroy(group)
    assert not err, err
    (i0, h0, l0, s0), (i1, h1, l1, s1) = out
    assert (i0["reason"], i0["nits"], i0["lits"]) == (i1["reason"], i1["nits"], i1["lits"])
    assert h0["trials"] == h1["trials"] and np.array_equal(h0["lam"], h1["lam"]) and np.array_equal(h0["fnorm"], h1["fnorm"])
    dl = max(abs(a - b)/abs(b) for a, b in zip(h0["lam"], ref["lam"]))
    dh = max(abs(a - b)/abs(b) for a, b in zip(h0["fnorm"], ref["hist"]))
    print("two slabs: reason", i0["reason"], "nits", i0["nits"], "lits", i0["lits"], "trials", h0["trials"], "max dev lambda %.3e ||F|| %.3e" % (dl, dh))
    assert (i0["reason"], i0["nits"], h0["trials"]) == (ref["reason"], ref["nits"], ref["trials"])
    assert l0["evaluations"] == l1["evaluations"] == ref["evaluations"] and l0["nonfinite"] == 0
    assert dl <= R.PARITY_TOL and dh <= R.PARITY_TOL, (dl, dh)
    un = np.concatenate([s0, s1], axis=1)
    for f in range(un.shape[0]):                           # (the state tolerance of tests/test_gpu_slabs.py: another stage 2, another path)
        assert rel2(un[f], ref["u"][f]) < 1e-7


def test_search_with_bicgstab():
    """Input A with the BiCGStab outer solver: the search only consumes dx."""
    spec, u0, ref = reference("A_order3")
    h = gpu_engine(spec, u0, {**R.A_OPTS, "linesearch": "bt", "ksp": "bcgs"}, 0.1)
    info = h.newton_solve()
    hist = h.ls_history()
    print("bcgs", info, list(hist["lam"]), hist["trials"])
    assert info["reason"] > 0 and info["fnorm"] <= R.A_OPTS["snes_rtol"]*info["fnorm0"]
    uh = h.get_state()
    for f in range(3):
        assert rel2(uh[f], ref["u"][f]) < 1e-6
    h.close()


def test_library_refuses_bad_search_options():
    """tp_create / tp_set_options name the field they refuse (the Python checks are bypassed by packing the struct directly)."""
    from thermalporous_amd import engine as E
    spec, u0, *_ = cases.c1_homogeneous(6, 1)
    h = E.HipEngine(spec, dict(pc="cpr"))
    base = E.resolve_ilu_options({**h.opts, "linesearch": "bt"}, spec["n"])
    bad = [("ls_order", dict(ls_order=4)), ("ls_alpha", dict(ls_alpha=0.5)), ("ls_alpha", dict(ls_alpha=0.0)), ("ls_max_it", dict(ls_max_it=0)),
           ("ls_maxstep", dict(ls_maxstep=0.0)), ("ls_minlambda", dict(ls_minlambda=1.0)), ("ls_minlambda", dict(ls_minlambda=-1.0))]
    for field, kw in bad:
        t = E.HipEngine._make_options({**base, **kw})
        assert h.lib.tp_set_options(h.ctx, C.byref(t)) != 0
        assert field in h.lib.tp_last_error().decode(), (field, h.lib.tp_last_error())
    for field, kw in [("ls_order", dict(ls_order=2)), ("ls_max_it", dict(ls_max_it=5)), ("ls_alpha", dict(ls_alpha=0.1)),
                      ("ls_maxstep", dict(ls_maxstep=2.0)), ("ls_minlambda", dict(ls_minlambda=1e-3)), ("ls_max_change", dict(ls_max_change=(0, 0, 0.1)))]:
        t = E.HipEngine._make_options({**base, **kw})
        t.ls_kind = 0                                          # a bt field away from its default under basic: refused, never ignored
        assert h.lib.tp_set_options(h.ctx, C.byref(t)) != 0
        assert field in h.lib.tp_last_error().decode(), (field, h.lib.tp_last_error())
    t = E.HipEngine._make_options({**base, "ls_order": 2, "ls_max_change": (1.0, 0.0, 0.2)})
    assert h.lib.tp_set_options(h.ctx, C.byref(t)) == 0
    t.ls_order = 5
    ctx = C.c_void_p()
    g = E.tp_grid(6, 6, 1, 1, 0, (C.c_double*3)(1.0, 1.0, 1.0), -1, 1, 0, 1)
    prm = E.tp_params(*[float(spec["prm"][k]) for k in E.tp_params._names])
    assert h.lib.tp_create(C.byref(g), C.byref(prm), C.byref(t), 0, C.byref(ctx)) != 0 and "ls_order" in h.lib.tp_last_error().decode()
    h.close()
