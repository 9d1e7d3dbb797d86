"""Inputs and independent checks for the Dirichlet sides.  The reference itself is ``oracle.tpfa.Problem`` with
``spec["boundary"]`` (or its ``boundary`` argument): {side: {"kind": "open" | "thermal", "p", "T", "S"}}, arrays shaped like the
side: (n_hi, n_lo) over the other two internal axes."""
import numpy as np

from oracle.tpfa import side_slice  # noqa: F401  (tests take it from here)


def side_shape(n, side):
    a = int(side)//2
    lo, hi = [k for k in range(3) if k != a]
    return (n[hi], n[lo])


def make_boundary(spec, u, kinds, seed=0):
    """Per-face ghost arrays for the sides in `kinds` ({side: "open" | "thermal"}) around the state `u`: p_b = the adjacent
    cell's p plus noise whose sign alternates from face to face (so a side of two or more faces has flow in both directions),
    T_b in 290..360, S_b in 0.05..0.95."""
    rng = np.random.default_rng(seed)
    u = np.asarray(u, dtype=float)
    n = tuple(int(v) for v in spec["n"])
    out = {}
    for side, kind in sorted(kinds.items()):
        shp = side_shape(n, side)
        nf = shp[0]*shp[1]
        sign = np.where((np.arange(nf) + side) % 2 == 0, 1.0, -1.0).reshape(shp)
        pc = u[0][side_slice(side)].reshape(shp)
        out[side] = {"kind": kind, "p": pc + sign*rng.uniform(0.3, 1.5, shp), "T": 290.0 + 70.0*rng.random(shp),
                     "S": 0.05 + 0.9*rng.random(shp) if spec["nphase"] == 2 else None}
    return out


def assert_both_directions(prob):
    """Every open side of `prob` (after a residual() call) has faces with Phi > 0 and faces with Phi <= 0 for each phase: a side
    that shows one direction only is an error of the test's inputs."""
    for side, B in prob.boundary.items():
        if B["kind"] != "open":
            continue
        for k, Phi in enumerate(prob.last_phi[side]):
            assert (Phi > 0.0).any() and (Phi <= 0.0).any(), ("one flow direction only", side, k)


def hydrostatic_column(nz=5):
    """A single-phase z column (internal axis 0 = z, gravity on it) at uniform p and T, and for its bottom (side 0) and top (side 1)
    the ghost pressure half a cell away on the hydrostat THROUGH the end cell's centre: dp/dz = -rho(p, T) g integrated with 2000
    midpoint steps by the oracle's closures -- no use of the face formula or of its factor g h/4.  Returns spec, u, {side: p_b}."""
    import cases
    from oracle import closures as cl
    spec, u0, prm, *_ = cases.c4_spe10_3d(Nx=1, Ny=1, Nz=nz, nphase=1)
    spec = dict(spec)
    spec["sources"] = None
    assert spec["gaxis"] == 0 and tuple(spec["n"]) == (nz, 1, 1)
    u = np.array(u0, dtype=float)
    g, h, API = spec["prm"]["g"], spec["h"][0], spec["prm"]["API"]
    pb = {}
    for side, cell, sgn in ((0, 0, -1.0), (1, nz - 1, 1.0)):      # z up: the bottom ghost lies h/2 below, the top one h/2 above
        p, T = float(u[0, 0, 0, cell]), float(u[1, 0, 0, cell])
        dz = sgn*0.5*h/2000
        for _ in range(2000):
            pm = p - 0.5*dz*g*cl.oil_rho(p, T, API)[0]
            p = p - dz*g*cl.oil_rho(pm, T, API)[0]
        pb[side] = p
    return spec, u, pb


def hydrostatic_boundary(spec, u, pb, shift=0.0):
    """Open bottom and top of hydrostatic_column at the hydrostatic ghost pressures (+ shift), ghost T = the cell's."""
    one = np.ones((1, 1))
    nz = spec["n"][0]
    return {side: {"kind": "open", "p": (pb[side] + shift)*one, "T": u[1, 0, 0, cell]*one, "S": None}
            for side, cell in ((0, 0), (1, nz - 1))}
