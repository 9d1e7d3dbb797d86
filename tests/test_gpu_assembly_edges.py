"""The assembly kernels (k_assemble, k_assemble_lds, k_accum_old, k_trans, k_trans_halo, k_sources of csrc/tp_assembly.hip)
at the states and fields the stage tests never reach (tests/edge_cases.py): saturations 0, 1, -0.05 and 1.05 next to each
other, exact upwind ties that carry information (gt, not ge), interior faces of zero transmissibility and zero conductivity,
porosity 0 and 1 -- entry by entry against the CPU oracle, on one slab and slab by slab, with test_assembly_parity's
assertions (1e-11 of the largest entry of the same field / block; rates rtol 1e-12).  The saturation guard
(tp_saturation_range / tp_clamp_saturation) gets its own tests.  Every input is finite and so is the oracle's output."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import cases
import edge_cases as ec
import switches

pytestmark = pytest.mark.gpu

TOL = 1e-11
PAIRS = ec.edge_pairs()


def _opts(nphase):
    return dict(pc="cptr" if nphase == 2 else "fieldsplit_cd")


def _oracle(spec, u, dt=8640.0):
    from oracle.engine import OracleEngine
    o = OracleEngine(spec, _opts(spec["nphase"]))
    o.set_old(u)
    o.set_dt(dt)
    o.set_state(u)
    R = o.residual()
    J, Sm = o.jacobian(want_schur=True)
    rates = o.well_rates()
    for a in (R, J, Sm) + tuple(rates.values()):
        assert np.isfinite(a).all()
        a.setflags(write=False)
    return R, J, Sm, rates


def assert_entries(Rh, Jh, Sh, Ro, Jo, So, tag=None):
    """test_assembly_parity's assertions on (a slab of) residual, Jacobian and S~; the scales are the oracle's over the same rows."""
    b = Ro.shape[0]
    for f in range(b):
        assert np.abs(Rh[f] - Ro[f]).max() < TOL*np.abs(Ro[f]).max(), (tag, "residual field", f)
    for r in range(b):
        for c in range(b):
            scale = np.abs(Jo[:, r, c]).max()
            if scale == 0.0:
                assert np.abs(Jh[:, r, c]).max() == 0.0
                continue
            assert np.abs(Jh[:, r, c] - Jo[:, r, c]).max() < TOL*scale, (tag, "J block", r, c)
    assert np.abs(Sh - So).max() < TOL*np.abs(So).max(), (tag, "S~")


@pytest.mark.parametrize("pid,name,builder,kw,kind", PAIRS, ids=[p[0] for p in PAIRS])
def test_edge_states_against_the_oracle(pid, name, builder, kw, kind):
    """Old state = the edge state itself: k_accum_old sees S outside [0, 1] too, and the residual shows it."""
    from thermalporous_amd.engine import HipEngine
    spec, u = ec.edge_input(builder, kw, kind)
    Ro, Jo, So, rates = _oracle(spec, u)
    if kind == "ties":
        # the reference takes ties to the '-' side and that can be seen: the other choice gives another energy row
        P = ec.PlusTieProblem(spec)
        P.set_old(u)
        P.set_dt(8640.0)
        Jp = P.jacobian(u)
        assert np.abs(Jp[:, 1, 0] - Jo[:, 1, 0]).max() > 1e-3*np.abs(Jo[:, 1, 0]).max()
    h = HipEngine(spec, _opts(kw["nphase"]))
    h.set_old(u)
    h.set_dt(8640.0)
    h.set_state(u)
    Rh = h.residual()
    Jh, Sh = h.jacobian(want_schur=True)
    assert_entries(Rh, Jh, Sh, Ro, Jo, So, pid)
    rh = h.well_rates()
    for k in rates:
        assert np.allclose(rh[k], rates[k], rtol=1e-12, atol=1e-30), k
    h.close()


# ---- slabs -----------------------------------------------------------------------------------------------------------------
def _on_slabs(spec, nranks, work):
    """`work(engine)` on every rank of an in-process slab group (one host thread per rank, as in tests/test_gpu_slabs.py)."""
    from thermalporous_amd import engine as E
    lib = E.load_library()
    group = C.c_void_p()
    assert lib.tp_local_group_create(nranks, C.byref(group)) == 0
    out, err = [None]*nranks, []

    def worker(rank):
        try:
            h = E.HipEngine(spec, _opts(spec["nphase"]), rank=rank, nranks=nranks, local_group=group)
            out[rank] = work(h)
            h.close()
        except Exception as e:      # noqa: BLE001
            err.append((rank, repr(e)))
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(nranks)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts), "slab worker hung"
    lib.tp_local_group_destroy(group)
    assert not err, err
    return out


def test_assembly_slab_by_slab():
    """3 slabs of 4, 4 and 3 planes; the middle slab has no source, the last one has sources in its first and in its last owned
    plane (and the first slab in both of its boundary planes): k_trans_halo, the off2 indexing, the remapping of source cells."""
    spec, *_ = cases.c4_spe10_3d(Nx=6, Ny=11, Nz=5, nphase=2)
    n0, n1, n2 = spec["n"]
    assert n2 == 11
    u = ec.edge_state(spec, 3, "sat")
    npl = n0*n1
    planes = [0, 3, 7 + 1, 10]                # slab 0: planes 0..3, slab 1: 4..7, slab 2: 8..10
    pool = np.concatenate([np.arange(k*npl, (k + 1)*npl) for k in planes])
    spec = ec.branch_sources(spec, 7, 40, u, cells=pool)
    ec.check_cap_margin(spec, u)
    src_planes = set((spec["sources"]["cell"]//npl).tolist())
    assert src_planes == set(planes)
    Ro, Jo, So, rates = _oracle(spec, u)

    def work(h):
        h.set_old(u)
        h.set_dt(8640.0)
        h.set_state(u)
        R = h.residual()
        J, Sm = h.jacobian(want_schur=True)
        return (h.lo, h.hi), R, J, Sm, h.well_rates(), h.src_index.copy(), h.saturation_range()
    out = _on_slabs(spec, 3, work)
    assert [o[0] for o in out] == [(0, 4), (4, 8), (8, 11)]
    seen = []
    for (lo, hi), R, J, Sm, rh, idx, srange in out:
        assert_entries(R, J, Sm, Ro[:, lo:hi], Jo[:, :, :, lo:hi], So[:, lo:hi], (lo, hi))
        if len(idx) == 0:
            assert rh == {}
        for k in rates:
            if len(idx):
                assert np.allclose(rh[k], rates[k][idx], rtol=1e-12, atol=1e-30), (k, lo)
        seen += idx.tolist()
        assert srange == (u[2, lo:hi].min(), u[2, lo:hi].max())
    assert sorted(seen) == list(range(len(spec["sources"]["cell"])))
    assert len(out[1][5]) == 0 and len(out[0][5]) > 0 and len(out[2][5]) > 0


# ---- saturation range and clamp ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last"])
def test_saturation_range_and_clamp_on_one_slab(where):
    from thermalporous_amd.engine import HipEngine
    spec, *_ = cases.c4_spe10_3d(Nx=6, Ny=7, Nz=5, nphase=2)
    u = cases.perturbed_state(spec, seed=3)
    S = u[2].reshape(-1)
    lo_at, hi_at = (0, S.size - 1) if where == "first" else (S.size - 1, 0)
    S[lo_at], S[hi_at] = -0.05, 1.05
    S[S.size//2], S[S.size//2 + 1] = 0.0, 1.0
    h = HipEngine(spec, dict(pc="cptr"))
    h.set_state(u)
    assert h.saturation_range() == (-0.05, 1.05)
    h.clamp_saturation()
    v = h.get_state()
    assert np.array_equal(v[2], np.clip(u[2], 0.0, 1.0))
    assert v[0].tobytes() == u[0].tobytes() and v[1].tobytes() == u[1].tobytes()
    assert h.saturation_range() == (0.0, 1.0)
    # one extreme only, in the one cell the other end of the array holds
    w = np.array(v)
    w[2].reshape(-1)[hi_at] = 1.05
    h.set_state(w)
    assert h.saturation_range() == (0.0, 1.05)
    h.close()


def test_saturation_range_is_that_of_the_owned_cells():
    """2 slabs: the global extremes of S lie in the neighbour's boundary plane, which is this slab's halo plane."""
    spec, *_ = cases.c4_spe10_3d(Nx=6, Ny=7, Nz=5, nphase=2)
    n0, n1, n2 = spec["n"]
    u = cases.perturbed_state(spec, seed=3)
    mid = (n2 + 1)//2                          # slab 0: planes 0..mid-1, slab 1: mid..n2-1
    u[2, mid, 0, 0], u[2, mid, -1, -1] = -0.05, 1.05
    expect = [(u[2, :mid].min(), u[2, :mid].max()), (-0.05, 1.05)]
    assert expect[0][0] >= 0.02 and expect[0][1] <= 0.98

    def work(h):
        h.set_state(u)
        before = h.saturation_range()
        h.clamp_saturation()
        return (h.lo, h.hi), before, h.get_state()
    out = _on_slabs(spec, 2, work)
    assert [o[0] for o in out] == [(0, mid), (mid, n2)]
    for r, ((lo, hi), before, v) in enumerate(out):
        assert before == expect[r], r
        assert np.array_equal(v[2], np.clip(u[2, lo:hi], 0.0, 1.0))
        assert v[:2].tobytes() == np.ascontiguousarray(u[:2, lo:hi]).tobytes()


# ---- the LDS-tiled variant ---------------------------------------------------------------------------------------------------
def _child(tmp, lds):
    """The arrays tests/asm_env_check.py wrote under TP_ASM_LDS=1, or with the switch unset (one run each, shared)."""
    return switches.run_child("asm_env_check.py", {"TP_ASM_LDS": "1"} if lds else {}, out=os.path.join(tmp, "asm_lds%d.npz" % lds),
                              timeout=300, cache=True)


@pytest.mark.parametrize("lds", [1, 0], ids=["lds", "default"])
def test_assembly_variant_matches_the_oracle_at_edge_states(lds, tmp_path_factory):
    """tests/asm_env_check.py in a fresh child process (TP_ASM_LDS is read once per process): every pair above on one slab."""
    _child(str(tmp_path_factory.getbasetemp()), lds)


def test_lds_tiled_assembly_is_bitwise_the_default(tmp_path_factory):
    """k_assemble_lds' header: "results are bitwise those of k_assemble" -- on partial tiles (none of the boxes is a multiple of
    16 x 4 x 4), one-cell-wide boxes and at the edge states.

    This test found the claim false while the LDS image held rho_o itself: 14 of the 96 arrays differed (J of 11 pairs, R of
    3, most of them "ties" pairs) in 1 to 81 entries each, by at most 4.9e-16 relative.  rho_o is a product that goes straight
    into the sum rho+ + rho- of the driving force; under -ffp-contract=fast k_assemble, which inlines eval_props, contracts the
    two into one fma, and a product rounded into the image first cannot be.  The image now holds the two factors."""
    tmp = str(tmp_path_factory.getbasetemp())
    a, b = _child(tmp, 1), _child(tmp, 0)
    assert sorted(a) == sorted(b) and len(a) == 3*len(PAIRS)
    bad = []
    for k in a:
        if a[k].tobytes() != b[k].tobytes():
            x, y = a[k].ravel(), b[k].ravel()
            d = x != y
            bad.append((k, int(d.sum()), float((np.abs(x - y)[d]/np.abs(y[d])).max())))
    print("arrays that differ (name, entries, largest relative difference):", bad)
    assert not bad, bad
