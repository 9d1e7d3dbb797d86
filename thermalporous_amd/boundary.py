"""Dirichlet sides of the box: open (flow and heat) and thermal (heat only) boundary faces.

Every side of a RectangleGeo / BoxGeo is closed to flow and to heat until ``geo.set_boundary`` sets it.  A boundary face is
an interior TPFA face whose other cell is a ghost state ``(p_b, T_b[, S_b])`` half a cell away, with the cell's own porosity
and static conductivity: same upwinding, gravity and harmonic conduction as inside.

    geo.set_boundary("z-", "thermal", T=params.T_prod)            # conduction into the base rock
    geo.set_boundary("x+", "open", p=p_aquifer, T=T_aquifer, S=1)   # an edge held at a given state

``build_spec`` maps what the geo holds through the internal axis order into ``spec["boundary"]``:
``{side_id: {"kind": "open" | "thermal", "p": a, "T": a, "S": a or None}}`` with ``side_id = 2*a + d`` (a the internal axis,
d = 0 its low-index side) and every array shaped ``(n_hi, n_lo)`` over the other two internal axes, the lower one fastest.
The key is absent when no side is set.
"""
import numpy as np

SIDES = {"x-": (0, 0), "x+": (0, 1), "y-": (1, 0), "y+": (1, 1), "z-": (2, 0), "z+": (2, 1)}
KINDS = {"none": 0, "open": 1, "thermal": 2}


def side_name(side_id, axes):
    """The physical name ("x-" ...) of internal side 2*a + d under the axis order `axes`."""
    a, d = divmod(int(side_id), 2)
    return "xyz"[axes[a]] + "-+"[d]


def _check_side(side, dim):
    if side not in SIDES:
        raise ValueError("unknown side %r: one of %s" % (side, ", ".join(sorted(SIDES))))
    if dim == 2 and SIDES[side][0] == 2:
        raise ValueError("side %r: a 2-D grid has no z sides" % (side,))


def _face_array(name, v, side, shape):
    """Scalar or array over the side's faces in physical order -> float array of `shape`, checked."""
    a = np.asarray(v, dtype=float)
    if a.ndim == 0:
        a = np.full(shape, float(a))
    else:
        squeezed = tuple(n for n in shape if n != 1) if a.ndim < len(shape) else shape
        if a.shape != shape and a.shape != squeezed:
            raise ValueError("%s on side %r has shape %r: a scalar or an array of shape %r over the side's faces"
                             % (name, side, a.shape, shape))
        a = a.reshape(shape).copy()
    if not np.isfinite(a).all():
        raise ValueError("%s on side %r holds a non-finite value" % (name, side))
    return a


def check_boundary(side, kind, p, T, S, N, dim):
    """One ``set_boundary`` call against the grid N = (Nx, Ny, Nz): the side, the kind, the shapes and the ranges.  Returns the
    values as arrays over the side's faces in physical order (None where not given)."""
    _check_side(side, dim)
    if kind not in KINDS:
        raise ValueError("boundary kind %r: 'open', 'thermal' or 'none'" % (kind,))
    if kind == "none":
        return None
    if T is None:
        raise ValueError("side %r, kind %r: the ghost temperature T is required" % (side, kind))
    pa = SIDES[side][0]
    shape = tuple(N[k] for k in range(3) if k != pa)
    out = {"kind": kind}
    for name, v in (("p", p), ("T", T), ("S", S)):
        out[name] = None if v is None else _face_array(name, v, side, shape)
    if out["S"] is not None and (out["S"].min() < 0.0 or out["S"].max() > 1.0):
        raise ValueError("S on side %r lies outside [0, 1]" % (side,))
    return out


def to_internal_side(side, entry, N, axes, nphase, params):
    """(side_id, spec entry) of one checked physical entry: defaults filled in, arrays in internal layout."""
    pa, d = SIDES[side]
    a = tuple(axes).index(pa)
    lo, hi = [k for k in range(3) if k != a]
    shape_phys = tuple(N[k] for k in range(3) if k != pa)
    kind = entry["kind"]
    p, T, S = entry["p"], entry["T"], entry["S"]
    if nphase == 2 and S is None:
        if kind == "open":
            raise ValueError("side %r: S is required for a two-phase open boundary (the ghost's mobilities follow it)" % (side,))
        S = np.full(shape_phys, float(params.S_o))          # thermal: it only sets the ghost's conductivity
    if p is None or kind == "thermal":
        p = np.full(shape_phys, float(params.p_ref))        # thermal: no flow through the face, p_b cannot matter
    # physical array (N[p1], N[p2]), p1 < p2  ->  internal (n_hi, n_lo)
    p1 = [k for k in range(3) if k != pa][0]
    flip = axes[hi] != p1

    def conv(v):
        return np.ascontiguousarray(v.T if flip else v)
    return 2*a + d, {"kind": kind, "p": conv(p), "T": conv(T), "S": conv(S) if nphase == 2 else None}


def boundary_spec(geo, params, nphase, axes):
    """``spec["boundary"]`` from what ``geo.set_boundary`` collected; {} when no side is set."""
    N = (geo.Nx, geo.Ny, geo.Nz)
    out = {}
    for side, entry in sorted(getattr(geo, "boundaries", {}).items()):
        sid, e = to_internal_side(side, entry, N, axes, nphase, params)
        out[sid] = e
    return out


def pack_values(entry, nphase):
    """The ghost state of one spec entry as the C ABI takes it: field-major (p_b, T_b[, S_b]), b * nfaces doubles."""
    f = [entry["p"], entry["T"]] + ([entry["S"]] if nphase == 2 else [])
    return np.ascontiguousarray(np.stack([np.asarray(v, dtype=float).reshape(-1) for v in f]))


class BoundaryMixin():
    """``set_boundary`` of RectangleGeo / BoxGeo."""

    def set_boundary(self, side, kind, p=None, T=None, S=None):
        """Set (or with kind "none" remove) the Dirichlet state of one side.

        side: "x-", "x+", "y-", "y+", "z-" or "z+" (the low / high end of the physical axis; z sides in 3-D only).
        kind: "open" (flow and conduction), "thermal" (conduction only) or "none".
        p, T, S: the ghost state, scalars or arrays over the side's faces in physical order -- "x-" takes (Ny, Nz), "y+"
        (Nx, Nz), "z-" (Nx, Ny); in 2-D (Ny,) and (Nx,).  T is required.  p defaults to ``params.p_ref`` and is ignored for
        "thermal".  S (two-phase only) is required for "open"; for "thermal" it defaults to ``params.S_o`` and only sets the
        ghost's conductivity.  Takes effect in models built afterwards (build_spec reads it)."""
        e = check_boundary(side, kind, p, T, S, (self.Nx, self.Ny, self.Nz), self.dim)
        if not hasattr(self, "boundaries"):
            self.boundaries = {}
        if e is None:
            self.boundaries.pop(side, None)
        else:
            self.boundaries[side] = e
