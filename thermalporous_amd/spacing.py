"""Graded tensor-product grids: one width per cell index along each axis.

A RectangleGeo / BoxGeo has ``N`` equal cells of ``Length/N`` along each axis until ``geo.set_spacing`` gives an axis widths of its
own -- thin layers next to a heater or a cap rock, columns refined towards a well:

    geo.set_spacing(z=geometric_widths(geo.Nz, geo.Length_z, 1.3, refine="both"))

The widths of an axis must be positive and sum to the axis length (1e-12 relative); an omitted axis stays uniform.  ``geo.Dx``,
``geo.Dy`` and ``geo.Dz`` stay the MEAN widths ``Length/N``; once spacing is set nothing uses them as the size of a cell: cell
centres, picking, well weights, volumes and the output coordinates come from the cumulative widths (``cell_edges``).  Spacing is
part of the grid a case picks its cells on, so it must be set before a case or a model is built from the geo.

``build_spec`` passes the widths on as ``spec["hs"]``, three arrays in internal axis order, only when spacing is set.
"""
import numpy as np

AXES = "xyz"


def geometric_widths(N, length, ratio, refine="low"):
    """N widths that sum to `length` exactly, each `ratio` times its neighbour moving away from the refined end.

    refine: "low" (the thinnest cell at the low-coordinate end), "high", or "both" (thin cells at both ends, growing towards the
    middle; with an odd N the middle cell is the single widest).  ratio >= 1; ratio = 1 gives equal widths."""
    N = int(N)
    if N < 1:
        raise ValueError("geometric_widths: N = %d" % N)
    if not (np.isfinite(ratio) and ratio >= 1.0):
        raise ValueError("geometric_widths: ratio = %r: the growth factor from one cell to the next, >= 1" % (ratio,))
    if not (np.isfinite(length) and length > 0.0):
        raise ValueError("geometric_widths: length = %r" % (length,))
    if refine not in ("low", "high", "both"):
        raise ValueError("geometric_widths: refine = %r: 'low', 'high' or 'both'" % (refine,))
    i = np.arange(N)
    if refine == "low":
        e = i
    elif refine == "high":
        e = N - 1 - i
    else:
        e = np.minimum(i, N - 1 - i)
    w = float(ratio)**e.astype(float)
    w = w*(float(length)/w.sum())
    # the rounding of the scaling goes into the widest cell, so that the sum is the length to the last bit
    for _ in range(4):
        d = float(length) - float(np.sum(w))
        if d == 0.0:
            break
        w[int(np.argmax(w))] += d
    return w


def check_widths(name, w, N, length):
    """One axis of a ``set_spacing`` call: N positive finite widths that sum to `length` to 1e-12 relative."""
    a = np.array(w, dtype=float).reshape(-1)
    if a.size != N:
        raise ValueError("set_spacing: %s has %d widths but the grid has %d cells along %s" % (name, a.size, N, name))
    if not np.isfinite(a).all() or (a <= 0.0).any():
        raise ValueError("set_spacing: the widths of %s must be positive and finite" % name)
    if abs(float(a.sum()) - float(length)) > 1e-12*abs(float(length)):
        raise ValueError("set_spacing: the widths of %s sum to %.17g, not to the axis length %.17g" % (name, a.sum(), length))
    return a


def lock_spacing(geo):
    """A case or a model has been built on the geo: its cells are picked, ``set_spacing`` is refused from here on."""
    geo.spacing_locked = True


class SpacingMixin():
    """``set_spacing`` and the per-cell geometry of RectangleGeo / BoxGeo."""

    def _lengths(self):
        return (self.Length, self.Length_y, getattr(self, "Length_z", 1.0))[:self.dim]

    def set_spacing(self, x=None, y=None, z=None):
        """Widths of the cells along x, y and (3-D) z: arrays of Nx, Ny, Nz positive numbers that sum to the axis length; an
        omitted axis stays uniform, and a call with no argument returns to the uniform grid.  Before any case or model is
        built from the geo."""
        if getattr(self, "spacing_locked", False):
            raise RuntimeError("set_spacing after a case or a model was built from this geo: the wells and heaters have picked "
                               "their cells on the old grid.  Set the spacing first")
        if z is not None and self.dim == 2:
            raise ValueError("set_spacing: a 2-D grid has no z axis")
        N = (self.Nx, self.Ny, self.Nz)
        L = self._lengths()
        new = {}
        for a, w in enumerate((x, y, z)[:self.dim]):
            if w is not None:
                new[a] = check_widths(AXES[a], w, N[a], L[a])
        self.spacing = new or None

    @property
    def graded(self):
        return getattr(self, "spacing", None) is not None

    def cell_widths(self):
        """(hx, hy, hz): the widths along each axis (hz = [1.0] in 2-D); equal entries Length/N on an axis without spacing."""
        N = (self.Nx, self.Ny, self.Nz)
        D = (self.Dx, self.Dy, self.Dz if self.dim == 3 else 1.0)
        sp = getattr(self, "spacing", None) or {}
        return tuple(sp[a].copy() if a in sp else np.full(N[a], float(D[a])) for a in range(3))

    def cell_edges(self):
        """Per axis of the grid's dimension the N + 1 coordinates of the cell edges, from 0 to the axis length."""
        N = (self.Nx, self.Ny, self.Nz)
        D = (self.Dx, self.Dy, self.Dz if self.dim == 3 else 1.0)
        L = self._lengths()
        sp = getattr(self, "spacing", None) or {}
        out = []
        for a in range(self.dim):
            if a in sp:
                e = np.concatenate(([0.0], np.cumsum(sp[a])))
                e[-1] = float(L[a])
            else:
                e = np.arange(N[a] + 1)*D[a]
            out.append(e)
        return out

    def centres_1d(self):
        """Per axis the cell-centre coordinates: (i + 1/2) D on a uniform axis (the uniform grid's own expression, bit for bit),
        the mid-points of the edges on an axis with spacing."""
        N = (self.Nx, self.Ny, self.Nz)
        D = (self.Dx, self.Dy, self.Dz if self.dim == 3 else 1.0)
        sp = getattr(self, "spacing", None) or {}
        edges = self.cell_edges() if sp else None
        return [0.5*(edges[a][:-1] + edges[a][1:]) if a in sp else (np.arange(N[a]) + 0.5)*D[a] for a in range(self.dim)]

    def cell_centres(self):
        return np.meshgrid(*self.centres_1d(), indexing="ij")

    def cell_volumes(self):
        """Volume of every cell, shape (Nx, Ny) or (Nx, Ny, Nz)."""
        hx, hy, hz = self.cell_widths()
        if self.dim == 2:
            return hx[:, None]*hy[None, :]
        return hx[:, None, None]*hy[None, :, None]*hz[None, None, :]
