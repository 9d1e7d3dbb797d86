"""Hand-built inputs for the rate branches of the source kernel and the edge states of the assembly, shared by the CPU
twins (test_cport.py, test_oracle_tpfa.py) and the GPU tests (test_gpu_sources.py, test_gpu_assembly_edges.py); and, in the
last section, the edge inputs of Dirichlet sides, graded grids and saturation functions with the matrix of their combinations
(test_gpu_assembly_combos.py; the conditions are asserted on the CPU by test_bc_host.py, test_graded_host.py, test_satfn_host.py).

Everything here is plain data handed to ``spec["sources"]`` / the fields of a spec; the case classes are not touched.
Each builder comes with the check of the condition that makes its comparison meaningful (``check_*``): the conditions are
met by the choice of inputs and asserted on the oracle, never by leaving an entry or a face out."""
import numpy as np

import cases
from oracle import closures as cl
from oracle.tpfa import Problem, PROD, INJ, HEATER, _lo, _hi

# saturation values a Newton iterate reaches and perturbed_state never produces
SAT_EDGES = (0.0, 1.0, -0.05, 1.05)
# one period of the flat-array pattern of edge_state("sat"): indices into SAT_EDGES, -1 keeps perturbed_state's value.  The
# period holds every unordered pair of the four values as flat neighbours (01 12 23 30 02 21 13), so on any box whose axis 0
# is longer than one cell each value meets each other one across a face; the 5 kept cells let every value meet an interior one
_SAT_PERIOD = (0, 1, 2, 3, 0, 2, 1, 3, -1, -1, -1, -1, -1)

# rate caps of the well branches: Peaceman rates of the lists below lie between ~1e-9 and ~1e-2 in magnitude (WI 1e-9..1e-7,
# total mobility 1/mu_o .. 1/mu_w, draw-down 10..30), so a cap of 1e3 is never reached and a cap of 1e-14 always is
CAP_FAR, CAP_TINY = 1.0e3, 1.0e-14


def _unit_rate(spec, kind, p, T, S, WI, bhp):
    """|Peaceman rate| of one open well entry by the oracle's closures (only used to place the caps away from it)."""
    mo = cl.oil_mu(T, spec["prm"]["API"])[0]
    if spec["nphase"] == 1:
        return abs(WI/mo*(bhp - p))
    mw = cl.water_mu(T)[0]
    if kind == PROD:
        return abs(WI*(S/mo + (1.0 - S)/mw)*(bhp - p))
    return abs(WI/mw*(bhp - p))


def branch_sources(spec, seed, ncells, u, cells=None):
    """A copy of `spec` whose sources are `ncells` groups (= distinct cells) cycling through every branch of source_eval at
    the state `u` (p near 41.4):
      0 producer, Peaceman (cap far away), bhp 30      4 injector, capped (cap tiny), bhp 70
      1 producer, capped (cap tiny), bhp 30            5 injector, shut, bhp 20
      2 producer, shut, bhp 60                         6 three entries in one cell: constant-rate producer, heater,
      3 injector, Peaceman, bhp 70                       constant-rate injector
                                                       7 a lone heater
    every weight drawn in [0.3, 1.7] without 1, every WI log-uniform in 1e-9..1e-7.  From 10 cells on, the last two cells
    hold instead: two producers with different bhp (one Peaceman, one capped), and a producer plus an injector whose bhp is
    EXACTLY that cell's p in `u` (the >= / <= tie of the shut-well conditional: both give 0).  `cells`: the cells to draw
    from (default: all); the number of groups is `ncells` in every case."""
    rng = np.random.default_rng(seed)
    N = int(np.prod(spec["phi"].shape))
    u = np.asarray(u, dtype=float).reshape(len(u), -1)
    pool = np.arange(N) if cells is None else np.asarray(cells, dtype=np.int64)
    chosen = rng.permutation(pool)[:ncells]
    assert len(chosen) == ncells and len(set(chosen.tolist())) == ncells
    ent = []

    def wt():
        w = rng.uniform(0.3, 1.7)
        return w if abs(w - 1.0) > 0.05 else w + 0.2

    def well(c, kind, bhp, cap, const=0):
        sign = -1.0 if kind == PROD else 1.0
        ent.append((int(c), kind, wt(), float(bhp), sign*cap, 10.0**rng.uniform(-9.0, -7.0), const))

    def heater(c):
        ent.append((int(c), HEATER, wt(), 0.0, 0.0, 0.0, 0))

    nextra = 2 if ncells >= 10 else 0
    for i, c in enumerate(chosen[:ncells - nextra]):
        k = i % 8
        if k == 0:
            well(c, PROD, 30.0, CAP_FAR)
        elif k == 1:
            well(c, PROD, 30.0, CAP_TINY)
        elif k == 2:
            well(c, PROD, 60.0, CAP_FAR)
        elif k == 3:
            well(c, INJ, 70.0, CAP_FAR)
        elif k == 4:
            well(c, INJ, 70.0, CAP_TINY)
        elif k == 5:
            well(c, INJ, 20.0, CAP_FAR)
        elif k == 6:
            well(c, PROD, 30.0, 10.0**rng.uniform(-7.0, -5.0), const=1)
            heater(c)
            well(c, INJ, 70.0, 10.0**rng.uniform(-7.0, -5.0), const=1)
        else:
            heater(c)
    if nextra:
        c = chosen[ncells - 2]
        well(c, PROD, 30.0, CAP_FAR)
        well(c, PROD, 35.0, CAP_TINY)
        c = chosen[ncells - 1]
        well(c, PROD, u[0, c], CAP_FAR)
        well(c, INJ, u[0, c], CAP_FAR)
    # (the entry list is deliberately NOT sorted by cell: both engines must group it themselves)
    order = rng.permutation(len(ent))
    ent = [ent[i] for i in order]
    out = dict(spec)
    out["sources"] = {
        "cell": np.array([e[0] for e in ent], dtype=np.int64),
        "kind": np.array([e[1] for e in ent], dtype=np.int32),
        "wt": np.array([e[2] for e in ent], dtype=float),
        "bhp": np.array([e[3] for e in ent], dtype=float),
        "max_rate": np.array([e[4] for e in ent], dtype=float),
        "WI": np.array([e[5] for e in ent], dtype=float),
        "const": np.array([e[6] for e in ent], dtype=np.int32),
    }
    return out


def check_cap_margin(spec, u):
    """For every well entry that is neither shut nor constant-rate, |Peaceman rate|/|max_rate| lies outside [0.5, 2] at `u`, so
    that another rounding of the rate (the GPU forms dd*WI/mu, the oracle WI/mu*dd) cannot flip the cap branch.  Returns the
    number of (Peaceman, capped, shut) well entries."""
    s = spec["sources"]
    u = np.asarray(u, dtype=float).reshape(len(u), -1)
    npea = ncap = nshut = 0
    for i in range(len(s["cell"])):
        kind, c = int(s["kind"][i]), int(s["cell"][i])
        if kind == HEATER or s["const"][i]:
            continue
        p, T = u[0, c], u[1, c]
        S = u[2, c] if spec["nphase"] == 2 else None
        dd = s["bhp"][i] - p
        if (kind == PROD and dd >= 0.0) or (kind == INJ and dd <= 0.0):
            nshut += 1
            continue
        ratio = _unit_rate(spec, kind, p, T, S, s["WI"][i], s["bhp"][i])/abs(s["max_rate"][i])
        assert np.isfinite(ratio) and not (0.5 <= ratio <= 2.0), (i, kind, ratio)
        if ratio < 0.5:
            npea += 1
        else:
            ncap += 1
    return npea, ncap, nshut


def sources_only(spec):
    """A copy of `spec` without any flux: K == 0 on all axes, kT == 0 and ko = kw = kr = 0, so that every transmissibility and
    every harmonic conductivity is 0 through its guard.  With dt = 1e40 the accumulation is ~1e-36 of its terms: R and the
    diagonal Jacobian block of a source cell are then the output of the source kernel alone."""
    out = dict(spec)
    sh = spec["phi"].shape
    out["K"] = [np.zeros(sh) for _ in range(3)]
    out["kT"] = np.zeros(sh)
    out["prm"] = dict(spec["prm"], ko=0.0, kw=0.0, kr=0.0)
    return out


SOURCES_ONLY_DT = 1.0e40


def edge_state(spec, seed, kind, tie_S=False):
    """"sat": perturbed_state with S set to 0, 1, -0.05 and 1.05 on interleaved strides of the flat array (_SAT_PERIOD).
    "ties": p constant on 2x2(x2) patches, T (and S) random: the faces inside a patch on a non-gravity axis have Phi == 0
    exactly, with different T on both sides.  "all_tie" (2-D): uniform p, random T and S.
    tie_S ("ties", two phases): S_o is patch-constant too, so that under a capillary pressure p_w = p - p_c(S_o) is constant on
    a patch and the water phase ties where the oil phase does; without it the states are bit for bit what they were."""
    u = cases.perturbed_state(spec, seed=seed)
    sh = spec["phi"].shape
    if kind == "sat":
        if spec["nphase"] == 2:
            S = u[2].reshape(-1)
            pat = np.array(_SAT_PERIOD)[np.arange(S.size) % len(_SAT_PERIOD)]
            for k, v in enumerate(SAT_EDGES):
                S[pat == k] = v
        return u
    if kind == "ties":
        rng = np.random.default_rng(seed + 1000)
        P = 41.369 + 2.0*rng.standard_normal(tuple(-(-n//2) for n in sh))
        i2, i1, i0 = np.meshgrid(*[np.arange(n)//2 for n in sh], indexing="ij")
        u[0] = P[i2, i1, i0]
        if tie_S and spec["nphase"] == 2:
            Sp = np.clip(0.5 + 0.3*np.random.default_rng(seed + 2000).standard_normal(P.shape), 0.02, 0.98)
            u[2] = Sp[i2, i1, i0]
        return u
    if kind == "all_tie":
        assert spec["n"][2] == 1 and spec["gaxis"] < 0
        u[0] = 41.369
        return u
    raise ValueError(kind)


def sat_pairs_across_faces(spec, u):
    """The set of unordered pairs of SAT_EDGES values that meet across some face of the box."""
    S = np.asarray(u)[2]
    pairs = set()
    for a in range(3):
        if spec["n"][a] == 1:
            continue
        lo, hi = S[_lo(a)].ravel(), S[_hi(a)].ravel()
        for x, y in zip(lo, hi):
            if x in SAT_EDGES and y in SAT_EDGES and x != y:
                pairs.add(frozenset((x, y)))
    return pairs


def check_ties(spec, u, min_share=0.10):
    """Every face has Phi == 0 exactly or |Phi| > 1e-9 max|p| (so that no rounding can move a face across the upwind switch),
    and on every non-gravity axis that has faces inside a patch at least `min_share` of the faces are exact ties with
    different T on both sides.  Returns the number of informative ties."""
    P = Problem(spec)
    u = P.as_fields(np.asarray(u, dtype=float))
    p, T, S = P.split(u)
    pr = P.props(p, T, S)
    pmax = np.abs(p).max()
    ninf = 0
    for a in range(3):
        if P.n[a] == 1:
            continue
        tie_all = None
        for (Lk, rk, ce, c0, to2) in P.phases():
            rho = pr[rk][0]
            Phi = P._phi_face(p[_lo(a)], p[_hi(a)], rho[_lo(a)], rho[_hi(a)], P.geom.gam(a))
            assert np.all((Phi == 0.0) | (np.abs(Phi) > 1e-9*pmax)), (a, rk)
            tie = Phi == 0.0
            tie_all = tie if tie_all is None else (tie_all & tie)
        if a != P.gaxis:
            inf = tie_all & (T[_lo(a)] != T[_hi(a)])
            assert inf.sum() >= min_share*inf.size, (a, int(inf.sum()), inf.size)
            ninf += int(inf.sum())
    return ninf


class PlusTieProblem(Problem):
    """The oracle with the upwind comparison made non-strict (ge instead of gt): an exact tie goes to the '+' side.  A tie is
    moved to the smallest positive number, which the strict comparison of the face loop then sends to '+'; every product
    with it underflows to 0, like the products with Phi == 0 themselves.  Used only to show that a tie carries information."""

    def _phi_face(self, *face):
        Phi = super()._phi_face(*face)
        return np.where(Phi == 0.0, np.nextafter(0.0, 1.0), Phi)


def dead_block(spec):
    """A copy of `spec` with K == 0 on all axes in an interior 2x2x2 block of cells (clipped to the box), phi == 0 in the
    block's first cell and phi == 1 in its last, and for nphase == 1 kT == 0 in the block: interior faces then take the
    `s > 0` == false branch of the transmissibility and (one phase) of the harmonic conductivity."""
    out = dict(spec)
    sh = spec["phi"].shape
    blk = tuple(slice(min(1, n - 1) if n > 2 else 0, (min(1, n - 1) if n > 2 else 0) + min(2, n)) for n in sh)
    out["K"] = [np.array(np.broadcast_to(k, sh), dtype=float) for k in spec["K"]]
    for k in out["K"]:
        k[blk] = 0.0
    phi = np.array(np.broadcast_to(spec["phi"], sh), dtype=float)
    first = tuple(s.start for s in blk)
    last = tuple(s.stop - 1 for s in blk)
    phi[first] = 0.0
    if last != first:
        phi[last] = 1.0
    out["phi"] = phi
    if spec["nphase"] == 1:
        kT = np.array(np.broadcast_to(spec["kT"], sh), dtype=float)
        kT[blk] = 0.0
        out["kT"] = kT
    return out


def per_cell_scales(prob, u, R, J):
    """Scales of the per-cell comparison of the source tests.  Residual: the largest |R| of the cell, or -- where that is
    smaller -- the size of the accumulation terms (acc * V/dt * weight) whose difference the residual of a cell without an
    open source is.  Jacobian: per row of the cell's diagonal block, the largest magnitude of that row."""
    u = prob.as_fields(np.asarray(u, dtype=float))
    w = np.array([prob.w0, 1.0, prob.w2][:prob.b]).reshape(-1, 1, 1, 1)
    acc = np.abs(prob.accum(*prob.split(u))*w*(prob.vol/prob.dt)).max(axis=0)
    rs = np.maximum(np.abs(R).max(axis=0), acc)
    js = np.abs(J[0]).max(axis=1)          # (b rows, cells)
    return rs, js


def per_cell_errors(prob, u, Ra, Ja, Rb, Jb):
    """Largest per-cell relative difference of residual and diagonal block (a against the reference b), see per_cell_scales."""
    rs, js = per_cell_scales(prob, u, Rb, Jb)
    eR = (np.abs(Ra - Rb)/rs).max()
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(Ja[0] - Jb[0])/js[:, None]
    q = np.where(js[:, None] == 0.0, np.where(Ja[0] == 0.0, 0.0, np.inf), q)
    return float(eR), float(q.max())


# ---- the boxes and (spec, state) pairs of the assembly edge tests (test_gpu_assembly_edges.py, asm_env_check.py) ------------
EDGE_BOXES = [
    ("c4_5x6x4", cases.c4_spe10_3d, dict(Nx=5, Ny=6, Nz=4)),
    ("c4_17x5x6", cases.c4_spe10_3d, dict(Nx=17, Ny=5, Nz=6)),        # the slab axis longer than four LDS tiles
    ("c4_6x5x17", cases.c4_spe10_3d, dict(Nx=6, Ny=5, Nz=17)),        # internal axis 0 (z) longer than the LDS tile's 16
    ("c3_9x11", cases.c3_spe10_2d, dict(Nx=9, Ny=11)),
    ("deg_1x5x7", cases.c4_spe10_3d, dict(Nx=1, Ny=5, Nz=7)),
    ("deg_2x2x2", cases.c4_spe10_3d, dict(Nx=2, Ny=2, Nz=2)),
]


def edge_pairs():
    """[(id, box name, builder, kw incl. nphase, kind)] for one and two phases: "sat" (two phases), "ties", "all_tie" (2-D), "dead"."""
    out = []
    for name, builder, kw in EDGE_BOXES:
        for nphase in (1, 2):
            kinds = (["sat"] if nphase == 2 else []) + ["ties"] + (["all_tie"] if builder is cases.c3_spe10_2d else []) + ["dead"]
            for kind in kinds:
                out.append(("%s_%dph_%s" % (name, nphase, kind), name, builder, dict(kw, nphase=nphase), kind))
    return out


def edge_input(builder, kw, kind, seed=3):
    """(spec, state) of one pair; the conditions that make the pair informative are asserted here, on the CPU."""
    spec, *_ = builder(**kw)
    if kind == "dead":
        spec = dead_block(spec)
        return spec, cases.perturbed_state(spec, seed=seed)
    u = edge_state(spec, seed, kind)
    if kind == "ties":
        assert check_ties(spec, u) > 0
    if kind == "all_tie":
        assert check_ties(spec, u, min_share=1.0) > 0
    return spec, u


# ---- Dirichlet sides, graded grids and saturation functions at edge states (test_gpu_assembly_combos.py) ---------------------
COMBO_DT = 8640.0
# The per-row bound of test_gpu_assembly_combos.py: max(1e-11, 10 x the largest per-row difference between the graded problem with sides'
# analytic and complex-step Jacobians at the inputs of row 3), which test_graded_host.py measures and compares with this value.
TOL_ROW = 1e-11


def combo_problem(spec):
    """The reference on the keys of `spec`: "hs" (graded), "boundary" (sides), "satfn" (curves)."""
    return Problem(spec)


def combo_reference(spec, u, dt=COMBO_DT):
    """(problem, R, J, S~) of the matching reference with old state = state; every output finite and read-only."""
    P = combo_problem(spec)
    P.set_old(u)
    P.set_dt(dt)
    R = P.residual(u)
    J, Sm = P.jacobian(u, want_schur=True)
    for a in (R, J, Sm, P.last_flux):
        assert np.isfinite(a).all()
    for a in (R, J, Sm):
        a.setflags(write=False)
    return P, R, J, Sm


def _capillary(spec):
    sat = spec.get("satfn")
    return sat is not None and sat.get("capillary") is not None


def satfn_state(spec, seed=3):
    """perturbed_state with the first three cells at S_o = Sr_o, S_o = 1 - Sr_w and the S_o at which Se_w = pc_se_min (the state
    of test_gpu_satfn's entry tests): every branch of every curve holds a cell."""
    from satfn_ref import DEFAULT
    sat = {**DEFAULT, **spec["satfn"]}
    u = cases.perturbed_state(spec, seed=seed)
    S = u[2].reshape(-1)
    D = 1.0 - sat["Sr_o"] - sat["Sr_w"]
    S[0], S[1], S[2] = sat["Sr_o"], 1.0 - sat["Sr_w"], 1.0 - sat["Sr_w"] - sat["pc_se_min"]*D
    return u


def _face_phis(P, u):
    """[(axis, [Phi of each phase over the interior faces])] by the reference's own driving force."""
    p, T, S = P.split(P.as_fields(np.asarray(u, dtype=float)))
    pr = P.props(p, T, S)
    out = []
    for a in range(3):
        if P.n[a] == 1:
            continue
        phis = []
        for (Lk, rk, ce, c0, to2) in P.phases():
            pp, rho = P._phase_pressure(rk, p, pr), pr[rk][0]
            phis.append(P._phi_face(pp[_lo(a)], pp[_hi(a)], rho[_lo(a)], rho[_hi(a)], P.geom.gam(a)))
        out.append((a, phis))
    return out


def check_combo_ties(spec, u, min_share=0.10):
    """check_ties on the reference that matches `spec`: its own half distances in the gravity head and, under saturation
    functions, the phase pressures.  Every face of every phase has Phi == 0 exactly or |Phi| > 1e-9 max|p|; on every non-gravity
    axis at least `min_share` of the faces tie in EVERY phase with different T on both sides."""
    P = combo_problem(spec)
    u = P.as_fields(np.asarray(u, dtype=float))
    pmax = np.abs(u[0]).max()
    ninf = 0
    for a, phis in _face_phis(P, u):
        tie_all = None
        for k, Phi in enumerate(phis):
            assert np.all((Phi == 0.0) | (np.abs(Phi) > 1e-9*pmax)), (a, k)
            tie_all = (Phi == 0.0) if tie_all is None else (tie_all & (Phi == 0.0))
        if a != P.gaxis:
            inf = tie_all & (u[1][_lo(a)] != u[1][_hi(a)])
            assert inf.sum() >= min_share*inf.size, (a, int(inf.sum()), inf.size)
            ninf += int(inf.sum())
    return ninf


def _open_lateral(spec, B):
    """The open sides of the boundary dict `B` that do not lie on the gravity axis."""
    return [s for s in sorted(B) if B[s]["kind"] == "open" and s//2 != spec["gaxis"]]


def _tie_faces(spec, side, nf):
    """ceil(nf/3) faces of the side, flat: those of the largest permeability along the side's axis, cells that hold a source
    last -- a tie shows in the cell's diagonal block in proportion to T^K against the accumulation and source terms of that
    cell, and SPE10's permeabilities span orders of magnitude.  make_boundary alternates the sign of p_b - p with the parity
    of face number + side; a face is passed over if it is the last one left of its parity, so both directions remain."""
    from bc_ref import side_slice
    a = side//2
    sh = spec["phi"].shape
    K = np.array(np.broadcast_to(spec["K"][a], sh), dtype=float)
    src = spec.get("sources")
    if src is not None and len(src["cell"]):
        K.reshape(-1)[np.asarray(src["cell"], dtype=np.int64)] *= 1e-30
    order = np.argsort(-K[side_slice(side)].reshape(-1), kind="stable")
    left = [int(np.sum((np.arange(nf) + side) % 2 == q)) for q in (0, 1)]
    tie = np.zeros(nf, dtype=bool)
    for f in order:
        q = int((f + side) % 2)
        if tie.sum() < -(-nf//3) and left[q] > 1:
            tie[f] = True
            left[q] -= 1
    return tie


def boundary_ties(spec, u, kinds, satfn=None, seed=4):
    """make_boundary's ghosts with, on every open side of a non-gravity axis, a third of the faces (_tie_faces) at p_b bitwise
    the adjacent cell's p -- and, with a capillary pressure in `satfn`, S_b bitwise the cell's S_o, so that both phases have
    Phi == 0.0 exactly -- and T_b 15 K away from the cell's T.  The other faces keep make_boundary's values."""
    from bc_ref import make_boundary, side_slice
    u = np.asarray(u, dtype=float)
    B = make_boundary(spec, u, kinds, seed=seed)
    cap = satfn is not None and satfn.get("capillary") is not None
    for side in _open_lateral(spec, B):
        e = B[side]
        shp = e["p"].shape
        tie = _tie_faces(spec, side, e["p"].size).reshape(shp)
        sl = side_slice(side)
        Tc = u[1][sl].reshape(shp)
        e["p"] = np.where(tie, u[0][sl].reshape(shp), e["p"])
        e["T"] = np.where(tie, Tc + np.where(Tc > 335.0, -15.0, 15.0), e["T"])
        if cap:
            e["S"] = np.where(tie, u[2][sl].reshape(shp), e["S"])
    return B


def check_boundary_ties(spec, u):
    """On the reference of `spec` (with its boundary): every face of every open side has Phi == 0 exactly or |Phi| > 1e-9 max|p|
    in each phase; every open side off the gravity axis has at least a third of its faces tied in every phase, with T_b at
    least 10 K from the cell's T, and faces of both flow directions in each phase; and the tie carries information: with p_b of
    the tied faces moved one ulp to the side that makes Phi > 0 (a few ulps where one rounds away in p - p_c), some row of the
    diagonal block of every tie cell moves by more than 1e-6 of that row's largest entry.  Returns the number of tied faces."""
    from bc_ref import side_slice
    P, R, J, Sm = combo_reference(spec, u)
    u = P.as_fields(np.asarray(u, dtype=float))
    pmax = np.abs(u[0]).max()
    B = P.boundary
    for side, e in B.items():
        if e["kind"] == "open":
            for k, Phi in enumerate(P.last_phi[side]):
                assert np.all((Phi == 0.0) | (np.abs(Phi) > 1e-9*pmax)), (side, k)
    lateral = _open_lateral(spec, B)
    assert lateral, "no open side off the gravity axis"
    scale = np.abs(J).max(axis=(0, 2))                       # (b rows, cells): the largest entry of each row
    n = 0
    for side in lateral:
        phis = P.last_phi[side]
        tie = np.all([Phi == 0.0 for Phi in phis], axis=0)
        assert tie.sum() > 0 and 3*tie.sum() >= tie.size, (side, int(tie.sum()), tie.size)
        for k, Phi in enumerate(phis):
            assert (Phi > 0.0).any() and (Phi < 0.0).any(), ("one flow direction only", side, k)
        Tc = u[1][side_slice(side)]
        assert np.all(np.abs(np.asarray(B[side]["T"]).reshape(tie.shape) - Tc)[tie] >= 10.0), side
        # One side at a time (a cell of a one-cell-thick box ties on both sides of an axis, and the two changes cancel).  The
        # lower index is '+': on a high side the cell is P and Phi = p - p_b, on a low side Phi = p_b - p.  Water's Phi is a
        # difference of p - p_c, in which one ulp of p_b can round away: such a face moves on, a few ulps at most.
        moved = {s: dict(e) for s, e in B.items()}
        for _ in range(8):
            pb = np.asarray(moved[side]["p"], dtype=float).reshape(tie.shape)
            Q = combo_problem(dict(spec, boundary=moved))
            Q.set_old(u)
            Q.set_dt(COMBO_DT)
            Q.residual(u)
            todo = tie & ~np.all([Phi > 0.0 for Phi in Q.last_phi[side]], axis=0)
            if not todo.any():
                break
            moved[side]["p"] = np.where(todo, np.nextafter(pb, -np.inf if side % 2 else np.inf), pb)
        Q, _, Jq, _ = combo_reference(dict(spec, boundary=moved), u)
        assert all(((Phi > 0.0) | ~tie).all() for Phi in Q.last_phi[side]), side
        assert np.abs(np.asarray(moved[side]["p"]) - np.asarray(B[side]["p"])).max() < 1e-13*pmax
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(scale > 0.0, np.abs(Jq[0] - J[0]).max(axis=1)/np.where(scale > 0.0, scale, 1.0), 0.0).max(axis=0)
        shown = rel[side_slice(side)][tie]
        assert np.all(shown > 1e-6), (side, shown.min())
        n += int(tie.sum())
    return n


_SIDE_SAT_PERIOD = (0, 1, 2, 3, -1)          # indices into SAT_EDGES over the cells of the open sides, -1 keeps the state's value


def boundary_sat_edges(spec, u, kinds, keep=(), offset=0, seed=4):
    """(state, boundary): the cells that lie on an open side, in flat order and without the flat cells `keep`, cycle through
    SAT_EDGES and the state's own value (period 5, started at `offset`); the ghosts cycle through S_b = 0.0, 1.0 and
    make_boundary's interior value with period 3, counted separately over the faces of each of the five cell values, so that a
    value that has two faces anywhere meets both ghost ends."""
    from bc_ref import make_boundary, side_slice
    assert spec["nphase"] == 2
    u = np.array(u, dtype=float)
    B = make_boundary(spec, u, kinds, seed=seed)
    on = np.zeros(u[2].shape, dtype=bool)
    for side, e in B.items():
        if e["kind"] == "open":
            on[side_slice(side)] = True
    S = u[2].reshape(-1)
    cells = [c for c in np.nonzero(on.reshape(-1))[0] if c not in keep]
    for k, c in enumerate(cells):
        v = _SIDE_SAT_PERIOD[(k + offset) % len(_SIDE_SAT_PERIOD)]
        if v >= 0:
            S[c] = SAT_EDGES[v]
    count = {}
    for side in sorted(B):
        e = B[side]
        if e["kind"] != "open":
            continue
        Sb = np.array(e["S"], dtype=float).reshape(-1)
        for f, x in enumerate(u[2][side_slice(side)].reshape(-1)):
            k = count.get(float(x) if x in SAT_EDGES else None, 0)
            count[float(x) if x in SAT_EDGES else None] = k + 1
            if k % 3 < 2:
                Sb[f] = float(k % 3)
        e["S"] = Sb.reshape(e["S"].shape)
    return u, B


def boundary_sat_pairs(spec, u):
    """The set of (cell's S_o in SAT_EDGES, S_b in {0, 1}) that occur on some face of an open side of spec["boundary"]."""
    from bc_ref import side_slice
    pairs = set()
    for side, e in spec["boundary"].items():
        if e["kind"] != "open":
            continue
        Sc = np.asarray(u)[2][side_slice(side)].ravel()
        for x, y in zip(Sc, np.asarray(e["S"], dtype=float).ravel()):
            if x in SAT_EDGES and y in (0.0, 1.0):
                pairs.add((float(x), float(y)))
    return pairs


ALL_SIDE_SAT_PAIRS = {(x, y) for x in SAT_EDGES for y in (0.0, 1.0)}


def check_boundary_sat_edges(spec, u, partial=False):
    """Every pair (cell value in SAT_EDGES, S_b in {0, 1}) occurs on some face of an open side; with saturation functions the
    cells at S_o = Sr_o and S_o = 1 - Sr_w of satfn_state (flat cells 0 and 1) lie on an open side and still hold those values.
    `partial` (the five-cell line under saturation functions, which cannot hold those two cells and the four edge values): at
    least two of the four edge values, each against both ghost values; test_satfn_host.py asserts that the line's cases
    together hold every pair.  Returns the set."""
    from bc_ref import side_slice
    pairs = boundary_sat_pairs(spec, u)
    if partial:
        assert len(pairs) >= 4 and all((x, 1.0 - y) in pairs for x, y in pairs), sorted(pairs)
    else:
        assert pairs == ALL_SIDE_SAT_PAIRS, sorted(ALL_SIDE_SAT_PAIRS - pairs)
    sat = spec.get("satfn")
    if sat is not None:
        on = np.zeros(np.asarray(u)[2].shape, dtype=bool)
        for side, e in spec["boundary"].items():
            if e["kind"] == "open":
                on[side_slice(side)] = True
        S = np.asarray(u)[2].reshape(-1)
        assert on.reshape(-1)[0] and on.reshape(-1)[1] and S[0] == sat["Sr_o"] and S[1] == 1.0 - sat["Sr_w"]
    return pairs


def dead_on_side(spec, side):
    """dead_block's 2x2x2 block moved along the axis of `side` until it touches that side: K == 0 on all axes in the block,
    phi == 0 in the block cell on the side (the first one in the other two directions), phi == 1 in that cell's inward
    neighbour (where the box is one cell thick along the axis: in the block's last cell), and for nphase == 1 kT == 0 in the
    block.  The boundary faces of the block then have T^K == 0 and, for one phase, no conduction either."""
    a, d = divmod(int(side), 2)
    out = dict(spec)
    sh = spec["phi"].shape
    ad = 2 - a                                               # the array dimension of internal axis a
    start = [(max(n - 2, 0) if d else 0) if k == ad else (min(1, n - 1) if n > 2 else 0) for k, n in enumerate(sh)]
    blk = tuple(slice(s, s + min(2, n)) for s, n in zip(start, sh))
    out["K"] = [np.array(np.broadcast_to(k, sh), dtype=float) for k in spec["K"]]
    for k in out["K"]:
        k[blk] = 0.0
    phi = np.array(np.broadcast_to(spec["phi"], sh), dtype=float)
    on = list(start)
    on[ad] = sh[ad] - 1 if d else 0
    inward = list(on)
    if sh[ad] > 1:
        inward[ad] += -1 if d else 1
    else:
        inward = [s.stop - 1 for s in blk]
    phi[tuple(on)] = 0.0
    if inward != on:
        phi[tuple(inward)] = 1.0
    out["phi"] = phi
    if spec["nphase"] == 1:
        kT = np.array(np.broadcast_to(spec["kT"], sh), dtype=float)
        kT[blk] = 0.0
        out["kT"] = kT
    return out


def check_dead_on_side(spec, side):
    """The side holds cells with K == 0 on every axis, among them one with phi == 0, and a cell with phi == 1 lies in the box;
    for one phase the dead cells on the side have kT == 0.  Returns whether EVERY cell of the side is dead."""
    from bc_ref import side_slice
    sl = side_slice(side)
    dead = np.all([np.asarray(k)[sl] == 0.0 for k in spec["K"]], axis=0)
    phi = np.asarray(spec["phi"])
    assert dead.any() and (phi[sl][dead] == 0.0).any(), side
    assert (phi == 1.0).any() or phi.size == 1
    if spec["nphase"] == 1:
        assert np.all(np.asarray(spec["kT"])[sl][dead] == 0.0)
    return bool(dead.all())


def no_conduction(spec):
    """A copy of `spec` with ko = kw = kr = 0 and (one phase) kT == 0: every thermal conductivity is 0, so every conduction
    denominator, interior and boundary, uniform (k+ + k-) and graded (c+ k- + c- k+), is 0 and each takes its guard's false
    branch, the guarded derivatives dH/dk of the two-phase code included."""
    out = dict(spec)
    out["prm"] = dict(spec["prm"], ko=0.0, kw=0.0, kr=0.0)
    if spec["nphase"] == 1:
        out["kT"] = np.zeros(spec["phi"].shape)
    return out


def check_no_conduction(spec, u):
    P = combo_problem(spec)
    kT = P.props(*P.split(P.as_fields(np.asarray(u, dtype=float))))["kT"][0]
    assert np.all(np.broadcast_to(kT, P.shape) == 0.0)


def per_row_errors(Jh, Sh, Jo, So):
    """Largest per-row relative difference of J (per cell and equation, over the 7 b entries of the row, against the largest
    reference entry of that row) and of S~ (per cell, over its 7 entries).  A row the reference has exactly zero must be exactly
    zero: it counts as inf otherwise."""
    def rel(d, s):
        with np.errstate(invalid="ignore", divide="ignore"):
            q = d/np.where(s > 0.0, s, 1.0)
        return float(np.where(s > 0.0, q, np.where(d == 0.0, 0.0, np.inf)).max())
    eJ = rel(np.abs(Jh - Jo).max(axis=(0, 2)), np.abs(Jo).max(axis=(0, 2)))
    eS = rel(np.abs(Sh - So).max(axis=0), np.abs(So).max(axis=0))
    return eJ, eS


def per_cell_residual_error(prob, u, Rh, Ro, Jo):
    """Largest per-cell difference of the residual in units of per_cell_scales' residual scale."""
    rs, _ = per_cell_scales(prob, u, Ro, Jo)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(Rh - Ro).max(axis=0)/np.where(rs > 0.0, rs, 1.0)
    return float(np.where(rs > 0.0, q, np.where(np.abs(Rh - Ro).max(axis=0) == 0.0, 0.0, np.inf)).max())


_C4, _C3 = cases.c4_spe10_3d, cases.c3_spe10_2d
MIXED_SIDES = {1: "open", 2: "open", 3: "thermal", 4: "open", 5: "open"}     # (side 0 stays closed; 1 is the top: gravity in Phi)
ALL_OPEN = {s: "open" for s in range(6)}
SIDES_2D = {0: "open", 1: "thermal", 2: "open", 3: "open"}
LATERAL_OPEN = {0: "thermal", 1: "thermal", 2: "open", 3: "open", 4: "open", 5: "open"}
COMBO_BOXES = {
    "2ph_6x5x4": (_C4, dict(Nx=6, Ny=5, Nz=4, nphase=2), MIXED_SIDES),
    "2ph_5x6x4": (_C4, dict(Nx=5, Ny=6, Nz=4, nphase=2), MIXED_SIDES),
    "1ph_5x6x4": (_C4, dict(Nx=5, Ny=6, Nz=4, nphase=1), MIXED_SIDES),
    "1ph_4x5x6_open": (_C4, dict(Nx=4, Ny=5, Nz=6, nphase=1), ALL_OPEN),
    "2ph_2d_7x5": (_C3, dict(Nx=7, Ny=5, nphase=2), SIDES_2D),
    "2ph_line_1x1x5": (_C4, dict(Nx=1, Ny=1, Nz=5, nphase=2), LATERAL_OPEN),        # five cells, each on all four lateral sides
    "2ph_2x2x2_open": (_C4, dict(Nx=2, Ny=2, Nz=2, nphase=2), ALL_OPEN),            # every cell carries three sides
    "2ph_17x5x6_open": (_C4, dict(Nx=17, Ny=5, Nz=6, nphase=2), ALL_OPEN),          # 330 boundary cells: two workgroups
}
# (row, graded, sides, models, boxes, the box of the row's geometric-width case)
COMBO_ROWS = [
    (1, False, True, (None,), ("2ph_6x5x4", "1ph_4x5x6_open", "2ph_2d_7x5"), None),
    (2, True, False, (None,), ("2ph_6x5x4", "1ph_5x6x4", "2ph_2d_7x5"), "2ph_6x5x4"),
    (3, True, True, (None,), ("2ph_6x5x4", "1ph_4x5x6_open", "2ph_2x2x2_open"), "2ph_6x5x4"),
    (4, False, True, ("M2",), ("2ph_6x5x4",), None),
    (5, True, False, ("M2",), ("2ph_5x6x4",), "2ph_5x6x4"),
    (6, True, True, ("M1", "M2", "M3"), ("2ph_6x5x4", "2ph_5x6x4", "2ph_line_1x1x5", "2ph_2x2x2_open"), "2ph_6x5x4"),
    (7, True, True, ("M2",), ("2ph_17x5x6_open",), "2ph_17x5x6_open"),
]
LINE_OFFSETS = {"M1": 0, "M2": 1, "M3": 3}      # the line's three free cells: edge values (0 1 2), (1 2 3), (3 keep 0) of SAT_EDGES


def combo_kinds(box, sides):
    """The edge kinds that apply to a box: "sat" and "boundary_sat_edges" need a saturation, "ties" a non-gravity axis with
    faces inside a patch (the line has none), "all_tie" the 2-D box without sides, the three boundary kinds a side."""
    nphase = COMBO_BOXES[box][1]["nphase"]
    kinds = (["sat"] if nphase == 2 else []) + ([] if "line" in box else ["ties"])
    kinds += (["all_tie"] if "2d" in box and not sides else []) + ["dead", "no_conduction"]
    if sides:
        kinds += ["boundary_ties"] + (["boundary_sat_edges"] if nphase == 2 else []) + ["dead_on_side"]
    return kinds


def combo_cases(rows=None):
    """[dict(id, row, box, graded, sides, model, kind)] of the matrix; graded is False, "random" or "geometric"."""
    out = []
    for row, graded, sides, models, boxes, geo in COMBO_ROWS:
        if rows is not None and row not in rows:
            continue
        for model in models:
            tag = "row%d%s" % (row, "_" + model if model else "")
            for box in boxes:
                for kind in combo_kinds(box, sides):
                    out.append(dict(id="%s_%s_%s" % (tag, box, kind), row=row, box=box, graded="random" if graded else False,
                                    sides=sides, model=model, kind=kind))
        if geo is not None:
            out.append(dict(id="row%d_%s_geometric" % (row, geo), row=row, box=geo, graded="geometric", sides=sides,
                            model=models[-1] if models[0] else None, kind="plain"))
    return out


def combo_dead_side(case):
    """The side that "dead_on_side" kills cells on: the highest open side, or the lowest one for one phase and in row 7."""
    kinds = COMBO_BOXES[case["box"]][2]
    opens = [s for s in sorted(kinds) if kinds[s] == "open"]
    return opens[0] if (case["box"].startswith("1ph") or case["row"] == 7) else opens[-1]


def combo_input(case, seed=3):
    """(spec, state) of one case of the matrix.  The conditions that make the case informative are asserted here, on the
    reference and on the CPU."""
    from bc_ref import make_boundary, side_slice
    from graded_ref import random_widths, spec_lengths
    from satfn_ref import DEFAULT, MODELS
    from thermalporous_amd.spacing import geometric_widths
    builder, kw, kinds = COMBO_BOXES[case["box"]]
    spec, *_ = builder(**kw)
    kind = case["kind"]
    if case["graded"]:
        hs = list(random_widths(spec["n"], spec_lengths(spec), 7))
        if case["graded"] == "geometric":
            a = max(range(3), key=lambda k: spec["n"][k])            # neighbour ratio 4 along the longest axis
            assert spec["n"][a] >= 5 and a != spec["gaxis"]
            hs[a] = geometric_widths(spec["n"][a], spec_lengths(spec)[a], 4.0, refine="low")
        spec["hs"] = tuple(hs)
    if case["model"]:
        spec["satfn"] = {**DEFAULT, **MODELS[case["model"]]}
    sat = spec.get("satfn")
    if kind == "dead":
        spec = dead_block(spec)
    elif kind == "no_conduction":
        spec = no_conduction(spec)
    elif kind == "dead_on_side":
        spec = dead_on_side(spec, combo_dead_side(case))
    if kind in ("sat", "ties", "all_tie"):
        u = edge_state(spec, seed, kind, tie_S=_capillary(spec))
    elif kind in ("dead", "dead_on_side"):
        # (where every cell is dead the oil row is the producer's term alone, which satfn_state's first cells would make 0)
        u = cases.perturbed_state(spec, seed=seed)
    else:
        u = satfn_state(spec, seed) if sat else cases.perturbed_state(spec, seed=seed)
    if case["sides"]:
        if kind == "boundary_ties":
            spec["boundary"] = boundary_ties(spec, u, kinds, sat, seed=seed + 1)
        elif kind == "boundary_sat_edges":
            line = sat is not None and "line" in case["box"]
            u, spec["boundary"] = boundary_sat_edges(spec, u, kinds, keep=(0, 1) if sat else (),
                                                     offset=LINE_OFFSETS[case["model"]] if line else 0, seed=seed + 1)
        else:
            spec["boundary"] = make_boundary(spec, u, kinds, seed=seed + 1)
    if kind == "ties":
        assert check_combo_ties(spec, u) > 0
    elif kind == "all_tie":
        assert check_combo_ties(spec, u, min_share=1.0) > 0
    elif kind == "no_conduction":
        check_no_conduction(spec, u)
    elif kind == "dead_on_side":
        check_dead_on_side(spec, combo_dead_side(case))
    elif kind == "boundary_ties":
        assert check_boundary_ties(spec, u) > 0
    elif kind == "boundary_sat_edges":
        check_boundary_sat_edges(spec, u, partial=sat is not None and "line" in case["box"])
    if case["graded"] == "geometric":
        # the cells of a side that contains the geometric axis differ by more than 100 x in width, face area and volume (the
        # box's sides are looked at in the rows without sides too: there the plane's cells are interior-face neighbours only)
        a = max(range(3), key=lambda k: spec["n"][k])
        assert spec["hs"][a].max() > 100.0*spec["hs"][a].min()
        side = [s for s in sorted(kinds) if kinds[s] == "open" and s//2 != a][0]
        assert kinds.get(2*a) == "open", (side, a)               # (and the thinnest cells lie on an open side of their own)
        h0, h1, h2 = spec["hs"]
        Vc = (h2[:, None, None]*h1[None, :, None]*h0[None, None, :])[side_slice(side)]
        assert Vc.max() > 100.0*Vc.min(), (Vc.max(), Vc.min())
    return spec, u
