"""Cell picking (mirror of /root/reference/thermalporous/utils.py:7-25) and DG0 delta helpers.

``GetNodeClosestToCoordinate`` scans dofs in order with a strict ``<`` (:14-18), i.e. the FIRST
dof at minimal distance wins.  Firedrake's dof numbering is not reproducible here, so ties
(common: e.g. ``test0`` wells at x=2 with Dx=2 are equidistant from centres 1 and 3) are broken
by this build's documented order: lowest flat index c = i + Nx*(j + Ny*k) (x fastest).
MATLAB export helpers (:27-49) are debug aids outside the hot path.
"""
import numpy as np


def cell_index(geo, i, j, k=0):
    return i + geo.Nx*(j + geo.Ny*k)


def _window_graded(geo, w, half, reach):
    """_window on a geo with spacing (geo.set_spacing): the cell containing the point comes from np.searchsorted on the cell
    edges, and where `reach` gives a physical distance per axis the window runs from the cell containing w - reach to the one
    containing w + reach, plus the same margin of `half[a]` cells on both sides.  Centres are slices of geo.centres_1d()."""
    edges, cen = geo.cell_edges(), geo.centres_1d()
    N = (geo.Nx, geo.Ny, geo.Nz)[:geo.dim]

    def cell_of(a, x):
        return min(max(int(np.searchsorted(edges[a], x, side="right")) - 1, 0), N[a] - 1)
    lo, hi, axes = [], [], []
    for a in range(geo.dim):
        r = 0.0 if reach is None else float(reach[a])
        lo.append(max(cell_of(a, w[a] - r) - half[a], 0))
        hi.append(min(cell_of(a, w[a] + r) + half[a] + 1, N[a]))
        axes.append(cen[a][lo[a]:hi[a]])
    return lo, hi, np.meshgrid(*axes, indexing="ij")


def _window(geo, w, half, reach=None):
    """Index ranges [lo, hi) per axis of the cells within `half[a]` cells of the cell containing the point w, and the
    cell-centre coordinates of that window (same expressions as geo.cell_centres(), so the values are bit-identical).
    Everything a well needs lies in such a window; evaluating the reference's whole-grid expressions on it instead of on
    every cell makes well set-up O(1) per well (42 wells on the 71.8 M-cell box of config 5: minutes -> milliseconds)."""
    if getattr(geo, "graded", False):
        return _window_graded(geo, w, half, reach)
    N = (geo.Nx, geo.Ny, geo.Nz)[:geo.dim]
    D = (geo.Dx, geo.Dy, getattr(geo, "Dz", 1.0))[:geo.dim]
    lo, hi, axes = [], [], []
    for a in range(geo.dim):
        i = min(max(int(np.floor(w[a]/D[a])), 0), N[a] - 1)
        lo.append(max(i - half[a], 0))
        hi.append(min(i + half[a] + 1, N[a]))
        axes.append((np.arange(lo[a], hi[a]) + 0.5)*D[a])
    return lo, hi, np.meshgrid(*axes, indexing="ij")


def GetNodeClosestToCoordinate(geo, coord):
    lo, hi, cc = _window(geo, coord, [2]*geo.dim)
    d2 = sum((c - w)**2 for c, w in zip(cc, coord))
    # first minimum in flat order (x fastest): transpose so that ravel() runs i fastest, as the whole-grid scan did; a
    # centre outside the +-2 window is farther away than every centre inside it by more than a cell size -- never a tie
    flat = np.transpose(d2, tuple(range(d2.ndim))[::-1]).ravel()
    m = int(np.argmin(np.sqrt(flat)))
    shape = [h - l for l, h in zip(lo, hi)]
    idx, rem = [], m
    for a in range(geo.dim):
        idx.append(lo[a] + rem % shape[a])
        rem //= shape[a]
    return int(cell_index(geo, *idx))


class Delta():
    """Sparse DG0 'delta' function: ``cells`` (flat indices) with ``values`` (the DG0 nodal values,
    normalised so that sum(values*|E|) = 1, wellcase.py:117-122).  ``vol``: |E|, one number, or on a geo with spacing the
    volume of each of ``cells``."""

    def __init__(self, cells, values, vol):
        self.cells = np.asarray(cells, dtype=np.int64)
        self.values = np.asarray(values, dtype=float)
        self.vol = vol

    @property
    def weights(self):
        return self.values*self.vol

    def dense(self, geo):
        out = np.zeros(geo.Nx*geo.Ny*geo.Nz)
        np.add.at(out, self.cells, self.values)
        return out


def cell_volume(geo, cells=None):
    """|E|: one number on a uniform geo; on a geo with spacing the volumes of the flat cell indices `cells` (all cells, x
    fastest, when None)."""
    if not getattr(geo, "graded", False):
        return geo.Dx*geo.Dy*(geo.Dz if geo.dim == 3 else 1.0)
    v = geo.cell_volumes()
    v = v.reshape(geo.Nx, geo.Ny, geo.Nz).transpose(2, 1, 0).reshape(-1)
    return v if cells is None else v[np.asarray(cells, dtype=np.int64)]


def well_delta(geo, w):
    """1/|E| at the nearest cell centre (wellcase.py:157-169): weight 1, whatever the cell's volume."""
    node = GetNodeClosestToCoordinate(geo, w)
    vol = cell_volume(geo, [node])
    return Delta([node], 1.0/vol if np.ndim(vol) else [1.0/vol], vol)


def well_circle(geo, w, radius, height=None):
    """Bump exp(-1/(r^2-d^2)) for d<r sampled at cell centres, normalised by its integral;
    3-D adds |z-zw| < height; falls back to well_delta when no centre is inside
    (wellcase.py:110-123,141-155).  Evaluated on the window of cells that can lie inside (see _window).  On a geo with spacing
    the integral is sum(vals*|E_c|) with the cells' own volumes, and the window reaches `radius` (`height`) to both sides by
    the cell edges."""
    if getattr(geo, "graded", False):
        half = [2]*geo.dim
        reach = [radius, radius] + ([height] if geo.dim == 3 else [])
    else:
        half = [int(np.ceil(radius/geo.Dx)) + 2, int(np.ceil(radius/geo.Dy)) + 2]
        if geo.dim == 3:
            half.append(int(np.ceil(height/geo.Dz)) + 2)
        reach = None
    lo, hi, cc = _window(geo, w, half, reach)
    d2 = (cc[0] - w[0])**2 + (cc[1] - w[1])**2
    inside = d2 < radius**2
    if geo.dim == 3:
        inside = inside & (np.abs(cc[2] - w[2]) < height)
    if not inside.any():
        return well_delta(geo, w)
    idx = np.nonzero(inside)
    vals = np.exp(-(1.0/(-d2[idx] + radius**2)))
    gidx = [ix + l for ix, l in zip(idx, lo)]
    cells = cell_index(geo, *gidx) if geo.dim == 3 else cell_index(geo, gidx[0], gidx[1])
    vol = cell_volume(geo, cells)
    normalise = (vals*vol).sum() if np.ndim(vol) else vals.sum()*vol
    if normalise == 0:
        return well_delta(geo, w)
    order = np.argsort(cells)
    return Delta(cells[order], (vals/normalise)[order], vol[order] if np.ndim(vol) else vol)
