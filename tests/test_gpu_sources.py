"""The source kernel (k_sources / source_eval of csrc/tp_assembly.hip) against the CPU oracle on hand-built source lists that
reach every branch of the rate laws (tests/edge_cases.py): Peaceman, capped and shut producers and injectors in one and two
phases, the exact bhp == p tie, constant rates, heaters, groups of 2 and 3 entries in one cell, weights other than 1 -- in
more groups than one workgroup of 64 threads holds, at saturations 0, 1, -0.05 and 1.05.

Sources in isolation: all fluxes are switched off (edge_cases.sources_only) and dt = 1e40, so R and the diagonal block of a
source cell are the kernel's output alone, and they are compared PER CELL: every residual entry relative to the largest
|R| of that cell (or the size of its accumulation terms where that is larger: a cell without an open source holds only their
rounding), every entry of the b x b diagonal block relative to the largest magnitude of its row, S~'s diagonal relative to
itself.  Bound: the project's entry tolerance 1e-11.

Where the bound comes from: the two CPU twins (oracle.tpfa in numpy, oracle/cport in C++: other compiler, other summation
and contraction) were compared on these very inputs with this very scaling before the kernel ever ran on them; they
disagree by at most
    two phases: residual 8.1e-19, diagonal block 2.95e-13, S~ diagonal 2.1e-16
    one phase:  residual 2.0e-16, diagonal block 3.7e-15,  S~ diagonal 2.5e-16
(70 groups; 1, 64 and 65 groups give the same or less).  The 2.95e-13 is dS of the water/oil split of a producer in a
cell of pure oil, where d q_w/dS = -mu_o/mu_w * rate carries the rounding of both viscosity laws times their ratio.
tests/test_cport.py::test_cport_matches_numpy_oracle_on_isolated_source_branches holds the twins to 1e-12.  The figure
does not exceed 1e-12, so the bound stays the project's 1e-11 and is not derived from it; nothing of it comes from the HIP
kernel's own output.  Rates: rtol 1e-12 as in test_assembly_parity."""
import functools

import numpy as np
import pytest

import cases
import edge_cases as ec

pytestmark = pytest.mark.gpu

BOX = dict(Nx=6, Ny=7, Nz=5)
TOL = 1e-11


@functools.lru_cache(maxsize=None)
def _base(nphase):
    spec, *_ = cases.c4_spe10_3d(nphase=nphase, **BOX)
    u = ec.edge_state(spec, 3, "sat")
    u.setflags(write=False)
    return spec, u


@functools.lru_cache(maxsize=None)
def _reference(nphase, ncells, isolated, seed=7):
    """(spec, state, oracle R, J, S~, rates), computed once per input and shared read-only."""
    from oracle.engine import OracleEngine
    spec0, u = _base(nphase)
    spec = ec.branch_sources(spec0, seed, ncells, u)
    ec.check_cap_margin(spec, u)
    if isolated:
        spec = ec.sources_only(spec)
    o = OracleEngine(spec, dict(pc="cptr" if nphase == 2 else "fieldsplit_cd"))
    o.set_old(u)
    o.set_dt(ec.SOURCES_ONLY_DT if isolated else 8640.0)
    o.set_state(u)
    R = o.residual()
    J, Sm = o.jacobian(want_schur=True)
    rates = o.well_rates()
    for a in (R, J, Sm) + tuple(rates.values()):
        assert np.isfinite(a).all()
        a.setflags(write=False)
    return spec, u, o.prob, R, J, Sm, rates


def _hip(spec, opts, u, dt):
    from thermalporous_amd.engine import HipEngine
    h = HipEngine(spec, opts)
    h.set_old(u)
    h.set_dt(dt)
    h.set_state(u)
    return h


def _assert_rates(h, rates):
    rh = h.well_rates()
    for k in rates:
        assert np.allclose(rh[k], rates[k], rtol=1e-12, atol=1e-30), k


def _assert_isolated(h, ref, schur):
    spec, u, prob, Ro, Jo, So, rates = ref
    Rh = h.residual()
    out = h.jacobian(want_schur=schur)
    Jh = out[0] if schur else out
    assert np.isfinite(Rh).all() and np.isfinite(Jh).all()
    # no flux anywhere: the off-diagonal planes are exactly 0
    assert np.abs(Jo[1:]).max() == 0.0 and np.abs(Jh[1:]).max() == 0.0
    # per cell (source cells and all others alike: a cell without sources holds the rounding of its accumulation only)
    eR, eJ = ec.per_cell_errors(prob, u, Rh, Jh, Ro, Jo)
    print("per-cell error: residual %.2e  diagonal block %.2e" % (eR, eJ))
    assert eR < TOL and eJ < TOL, (eR, eJ)
    if schur:
        Sh = out[1]
        assert np.abs(So[1:]).max() == 0.0 and np.abs(Sh[1:]).max() == 0.0
        eS = (np.abs(Sh[0] - So[0])/np.abs(So[0])).max()
        print("per-cell error: S~ diagonal %.2e" % eS)
        assert eS < TOL, eS
    _assert_rates(h, rates)


ISOLATED = [(2, "cptr"), (2, "cpr"), (1, "fieldsplit_cd"), (1, "cpr")]


@pytest.mark.parametrize("nphase,pc", ISOLATED, ids=["%dph_%s" % c for c in ISOLATED])
def test_sources_in_isolation(nphase, pc):
    """70 groups (91 entries): the second workgroup runs and is partial; every branch, per cell."""
    ref = _reference(nphase, 70, True)
    spec, u = ref[0], ref[1]
    assert len(np.unique(spec["sources"]["cell"])) == 70 > 64
    if nphase == 2:
        assert set(ec.SAT_EDGES) <= set(u[2].reshape(-1)[spec["sources"]["cell"]])
    h = _hip(spec, dict(pc=pc), u, ec.SOURCES_ONLY_DT)
    _assert_isolated(h, ref, schur=pc in ("cptr", "fieldsplit_cd"))
    h.close()


@pytest.mark.parametrize("nphase", [1, 2])
def test_source_group_counts_at_the_workgroup_boundary(nphase):
    """1, 64 and 65 groups: one thread, exactly one full workgroup, one thread in the second.  One engine, sources re-set."""
    h = None
    for ncells in (1, 64, 65):
        ref = _reference(nphase, ncells, True)
        spec, u = ref[0], ref[1]
        assert len(np.unique(spec["sources"]["cell"])) == ncells
        if h is None:
            h = _hip(spec, dict(pc="cptr" if nphase == 2 else "fieldsplit_cd"), u, ec.SOURCES_ONLY_DT)
        else:
            h._set_sources(spec["sources"])
        _assert_isolated(h, ref, schur=True)
    h.close()


def _assert_planes(h, ref, schur=True):
    """test_assembly_parity's assertions: every field / block scaled by its largest entry over all planes."""
    spec, u, prob, Ro, Jo, So, rates = ref
    Rh = h.residual()
    Jh, Sh = h.jacobian(want_schur=True)
    b = prob.b
    for f in range(b):
        assert np.abs(Rh[f] - Ro[f]).max()/np.abs(Ro[f]).max() < TOL, ("residual field", f)
    for r in range(b):
        for c in range(b):
            scale = np.abs(Jo[:, r, c]).max()
            if scale == 0.0:
                assert np.abs(Jh[:, r, c]).max() == 0.0
                continue
            assert np.abs(Jh[:, r, c] - Jo[:, r, c]).max()/scale < TOL, ("J block", r, c)
    assert np.abs(Sh - So).max()/np.abs(So).max() < TOL
    _assert_rates(h, rates)


@pytest.mark.parametrize("nphase", [1, 2])
def test_sources_inside_the_full_operator(nphase):
    ref = _reference(nphase, 70, False)
    h = _hip(ref[0], dict(pc="cptr" if nphase == 2 else "fieldsplit_cd"), ref[1], 8640.0)
    _assert_planes(h, ref)
    h.close()


@pytest.mark.parametrize("nphase", [1, 2])
def test_resetting_sources_on_a_live_engine(nphase):
    """tp_set_sources a second time with another, shorter list and then with none: residual, Jacobian, S~ and rates follow."""
    from oracle.engine import OracleEngine
    ref = _reference(nphase, 70, False)
    spec, u = ref[0], ref[1]
    opts = dict(pc="cptr" if nphase == 2 else "fieldsplit_cd")
    h = _hip(spec, opts, u, 8640.0)
    _assert_planes(h, ref)
    ref2 = _reference(nphase, 23, False, 11)
    assert set(ref2[0]["sources"]["cell"]) != set(spec["sources"]["cell"])
    h._set_sources(ref2[0]["sources"])
    _assert_planes(h, ref2)
    none = dict(spec, sources=None)
    o = OracleEngine(none, opts)
    o.set_old(u)
    o.set_dt(8640.0)
    o.set_state(u)
    J, Sm = o.jacobian(want_schur=True)
    h._set_sources({k: v[:0] for k, v in spec["sources"].items()})
    assert h.well_rates() == {} and o.well_rates() == {}
    _assert_planes(h, (none, u, o.prob, o.residual(), J, Sm, {}))
    h.close()
