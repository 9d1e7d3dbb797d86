"""Inputs and independent checks for the graded tensor-product grid.  The reference itself is
``oracle.tpfa.Problem`` with ``spec["hs"]`` (or its ``hs`` argument): one width per cell index along each internal axis."""
import numpy as np

from oracle.tpfa import Problem


def random_widths(n, lengths, seed=0):
    """Per axis n[a] widths drawn from a seeded uniform(0.4, 2.5) and rescaled to sum to lengths[a]."""
    rng = np.random.default_rng(seed)
    out = []
    for a in range(3):
        w = rng.uniform(0.4, 2.5, int(n[a]))
        out.append(w*(float(lengths[a])/w.sum()))
    return tuple(out)


def equal_widths(spec):
    return tuple(np.full(int(spec["n"][a]), float(spec["h"][a])) for a in range(3))


def spec_lengths(spec):
    return tuple(float(spec["h"][a])*int(spec["n"][a]) for a in range(3))


def cell_centres_internal(hs):
    """Centre coordinates along each internal axis from the cumulative widths."""
    return tuple(np.cumsum(w) - 0.5*w for w in hs)


def hydrostatic_graded_column(props=(1.0, 4.0, 2.0, 8.0, 1.0, 4.0)):
    """A single-phase z column 1x1xN (internal axis 0 = z, gravity on it) with widths proportional to `props`, uniform T, and at
    the cell centres the pressure of the hydrostat dp/dz = -rho(p, T) g, integrated from the bottom centre upwards with 4000
    midpoint steps per interval between two centres by the oracle's closures: no use of the face formula or of its distance.
    Returns spec (with "hs", no sources), u, and per interior face the scale T^K L rho g d of the flux the gravity head alone
    would drive (d the distance between the two centres, the properties those of the lower cell)."""
    import cases
    from oracle import closures as cl
    nz = len(props)
    spec, u0, prm, *_ = cases.c4_spe10_3d(Nx=1, Ny=1, Nz=nz, nphase=1)
    spec = dict(spec)
    spec["sources"] = None
    assert spec["gaxis"] == 0 and tuple(spec["n"]) == (nz, 1, 1)
    w = np.asarray(props, dtype=float)
    eq = equal_widths(spec)
    spec["hs"] = (w*(spec_lengths(spec)[0]/w.sum()), eq[1], eq[2])
    z = cell_centres_internal(spec["hs"])[0]
    u = np.array(u0, dtype=float)
    g, API = spec["prm"]["g"], spec["prm"]["API"]
    T = float(u[1, 0, 0, 0])
    p = float(u[0, 0, 0, 0])
    for i in range(1, nz):
        dz = (z[i] - z[i - 1])/4000
        for _ in range(4000):
            pm = p - 0.5*dz*g*cl.oil_rho(p, T, API)[0]
            p = p - dz*g*cl.oil_rho(pm, T, API)[0]
        u[0, 0, 0, i] = p
    u[1] = T
    P = Problem(spec)
    pr = P.props(u[0], u[1], None)
    lo = (0, 0, slice(None, -1))
    scale = P.TK[0][lo]*pr["Lo"][0][lo]*pr["ro"][0][lo]*g*np.diff(z)
    return spec, u, np.asarray(scale, dtype=float).reshape(-1)


def field_change(Ra, Rb, spec):
    """Per field ||Ra - Rb|| / ||Rb|| over the cells that carry no well or heater entry: a source term is orders of magnitude
    above the face fluxes and does not depend on the spacing, so with those cells in, no norm would show the faces."""
    mask = np.ones(int(np.prod(Rb.shape[1:])), dtype=bool)
    src = spec.get("sources")
    if src is not None and len(src["cell"]):
        mask[np.asarray(src["cell"], dtype=np.int64)] = False
    assert mask.sum() >= 2
    out = []
    for f in range(Rb.shape[0]):
        a, b = Ra[f].reshape(-1)[mask], Rb[f].reshape(-1)[mask]
        out.append(float(np.linalg.norm(a - b)/np.linalg.norm(b)))
    return out
