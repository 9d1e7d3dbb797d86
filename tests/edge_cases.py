"""Hand-built inputs for the rate branches of the source kernel and the edge states of the assembly, shared by the CPU
twins (test_cport.py, test_oracle_tpfa.py) and the GPU tests (test_gpu_sources.py, test_gpu_assembly_edges.py).

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


def edge_state(spec, seed, kind):
    """"sat": perturbed_state with S set to 0, 1, -0.05 and 1.05 on interleaved strides of the flat array (_SAT_PERIOD).
    "ties": p constant on 2x2(x2) patches, T (and S) random: the faces inside a patch on a non-gravity axis have Phi == 0
    exactly, with different T on both sides.  "all_tie" (2-D): uniform p, random T and S."""
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
            Phi = P._phi_face(a, p, pr[rk][0])
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

    def _phi_face(self, a, p, rho):
        Phi = super()._phi_face(a, p, rho)
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
    acc = np.abs(prob.accum(*prob.split(u))*w*(prob.V/prob.dt)).max(axis=0)
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
