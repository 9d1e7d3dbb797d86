"""Completed wells: a well perforates a row of cells, shares one bottom-hole pressure along its bore, sees the hydrostatic head
between its perforations, and is operated at a total rate until its BHP limit is reached, then at that limit (DESIGN.md 4.1.4;
include/thermalporous_hip.h: tp_set_wells).  The reference's wells (wellcase.py) are deltas on single cells with a private bhp
each; they stay what they are, and a ``CompletedWellCase`` passes an existing case's entries through untouched.

The connection index comes from the TRUE geometry of each perforated cell (Peaceman, anisotropic form):
    r_o = 0.28 sqrt(sqrt(K_b/K_a) D_a^2 + sqrt(K_a/K_b) D_b^2) / ((K_b/K_a)^(1/4) + (K_a/K_b)^(1/4))
    WI  = 2 pi L sqrt(K_a K_b) / (ln(r_o / r_w) + skin)
with a, b the two axes across the well, D the perforated cell's own widths along them (on a graded grid: of that cell), K the
cell's permeabilities along them and L its width along the well axis.  A 2-D grid has unit thickness and the one cross
permeability it has in both cross directions.  The hard-coded constants of ``wellcase.peaceman_WI`` stay with the existing cases.
"""
import numpy as np

from .spacing import lock_spacing

AXES = {"x": 0, "y": 1, "z": 2}


def connection_index(Ka, Kb, Da, Db, L, radius=0.1, skin=0.0):
    """Peaceman's index of one perforation (arrays broadcast)."""
    Ka, Kb, Da, Db, L = (np.asarray(v, dtype=float) for v in (Ka, Kb, Da, Db, L))
    ro = 0.28*np.sqrt(np.sqrt(Kb/Ka)*Da**2 + np.sqrt(Ka/Kb)*Db**2)/((Kb/Ka)**0.25 + (Ka/Kb)**0.25)
    if np.any(ro <= radius):
        raise ValueError("well radius %g is not smaller than Peaceman's radius %g of a perforated cell" % (radius, float(np.min(ro))))
    return 2.0*np.pi*L*np.sqrt(Ka*Kb)/(np.log(ro/radius) + skin)


class CompletedWellCase():

    def __init__(self, params, geo, base=None):
        self.name = "Completed wells" + (" + " + base.name if base is not None and hasattr(base, "name") else "")
        self.params = params
        self.geo = geo
        self.base = base
        lock_spacing(geo)             # the wells below pick their cells on the grid as it is now
        self.wells = []

    def __getattr__(self, key):       # (only what this class does not define: init_IC, prod_wells, ... of the base case)
        base = self.__dict__.get("base")
        if base is None or key.startswith("__"):
            raise AttributeError(key)
        return getattr(base, key)

    # ---- the existing case's sources pass through untouched ----------------------------------------
    def source_entries(self):
        return self.base.source_entries() if hasattr(self.base, "source_entries") else []

    def heater_entries(self):
        return self.base.heater_entries() if hasattr(self.base, "heater_entries") else []

    # ---- geometry ----------------------------------------------------------------------------------
    def _fields(self):
        geo = self.geo
        N = (geo.Nx, geo.Ny, geo.Nz)

        def full(f):
            a = np.asarray(f, dtype=float)
            return np.full(N, float(a)) if a.ndim == 0 else a.reshape(N)
        K = [full(geo.K_x), full(geo.K_y)]
        K.append(full(geo.K_z) if geo.dim == 3 and hasattr(geo, "K_z") else None)
        return N, K, geo.cell_widths(), geo.centres_1d()

    def _pick(self, axis, xy, span, cells):
        geo = self.geo
        N, K, widths, cen = self._fields()
        a = AXES[axis]
        if cells is not None:
            idx = []
            for c in cells:
                if np.ndim(c) == 0:
                    c = int(c)
                    c = (c % N[0], (c//N[0]) % N[1], c//(N[0]*N[1]))
                c = tuple(int(v) for v in c) + (0,)*(3 - len(c))
                if not all(0 <= c[d] < N[d] for d in range(3)):
                    raise ValueError("cell %r lies outside the grid %r" % (c, N))
                idx.append(c)
            if not idx:
                raise ValueError("a well needs at least one cell")
            return idx
        cross = [d for d in range(3) if d != a]
        if xy is None or len(xy) != 2:
            raise ValueError("xy: the two coordinates across the well axis %r (in the order %s)" % (axis, ", ".join("xyz"[d] for d in cross)))
        fixed = {}
        for d, v in zip(cross, xy):
            fixed[d] = 0 if d >= geo.dim else int(np.argmin(np.abs(cen[d] - float(v))))
        if a >= geo.dim:
            along = [0]
        else:
            if span is None or len(span) != 2:
                raise ValueError("z: the range (lo, hi) along the well axis %r that the well is open over" % axis)
            lo, hi = float(min(span)), float(max(span))
            along = [i for i in range(N[a]) if lo <= cen[a][i] <= hi]
            if not along:
                raise ValueError("no cell centre of axis %r lies in [%g, %g]" % (axis, lo, hi))
        idx = []
        for i in along:
            c = [0, 0, 0]
            c[a] = i
            for d in cross:
                c[d] = fixed[d]
            idx.append(tuple(c))
        return idx

    def _add(self, kind, name, xy, z, cells, axis, rate, bhp, radius, skin, z_ref):
        if axis not in AXES:
            raise ValueError("axis = %r: 'x', 'y' or 'z'" % (axis,))
        if name in [w["name"] for w in self.wells]:
            raise ValueError("two wells are called %r" % (name,))
        if rate is None or bhp is None:
            raise ValueError("well %r: rate (the total rate target, >= 0) and bhp (the limit) are required" % (name,))
        if not (np.isfinite(rate) and np.isfinite(bhp)) or rate < 0:
            raise ValueError("well %r: rate = %r, bhp = %r: a finite rate >= 0 and a finite limit" % (name, rate, bhp))
        if not (radius > 0 and np.isfinite(skin)):
            raise ValueError("well %r: radius = %r, skin = %r" % (name, radius, skin))
        geo = self.geo
        N, K, widths, cen = self._fields()
        a = AXES[axis]
        idx = self._pick(axis, xy, z, cells)
        taken = {c: w["name"] for w in self.wells for c in w["ijk"]}
        for c in idx:
            if c in taken:
                raise ValueError("well %r: cell %r is already perforated by well %r" % (name, c, taken[c]))
        if len(set(idx)) != len(idx):
            raise ValueError("well %r lists a cell twice" % (name,))
        ca, cb = [d for d in range(3) if d != a]
        WI, zs, flat = [], [], []
        for c in idx:
            def Kof(d):
                if K[d] is not None:
                    return K[d][c]
                other = cb if d == ca else ca          # 2-D: the missing direction takes the other cross permeability
                return (K[other] if K[other] is not None else K[0])[c]
            Da, Db, L = widths[ca][c[ca]], widths[cb][c[cb]], widths[a][c[a]]
            WI.append(float(connection_index(Kof(ca), Kof(cb), Da, Db, L, radius, skin)))
            zs.append(float(cen[2][c[2]]) if geo.dim == 3 else 0.0)
            flat.append(c[0] + N[0]*(c[1] + N[1]*c[2]))
        self.wells.append({"name": str(name), "kind": kind, "rate": float(rate), "bhp": float(bhp), "shut": False,
                           "z_ref": float(max(zs) if z_ref is None else z_ref), "axis": axis, "ijk": idx,
                           "cells": np.array(flat, dtype=np.int64), "WI": np.array(WI), "z": np.array(zs)})
        return self.wells[-1]

    def add_producer(self, name, xy=None, z=None, cells=None, axis="z", rate=None, bhp=None, radius=0.1, skin=0.0, z_ref=None):
        """A producer open over the cells of the line through `xy` (the two coordinates across `axis`) whose centres lie in the
        range `z` = (lo, hi) along the axis, or over the listed `cells` ((ix, iy[, iz]) or flat x-fastest indices).  rate: the
        total volumetric rate target (>= 0, the units of params.rate); bhp: the minimum bottom-hole pressure."""
        return self._add("prod", name, xy, z, cells, axis, rate, bhp, radius, skin, z_ref)

    def add_injector(self, name, xy=None, z=None, cells=None, axis="z", rate=None, bhp=None, radius=0.1, skin=0.0, z_ref=None):
        """An injector; bhp is the maximum bottom-hole pressure."""
        return self._add("inj", name, xy, z, cells, axis, rate, bhp, radius, skin, z_ref)

    def well_entries(self):
        """The wells for ``build_spec``: dicts with name, kind, rate, bhp, z_ref, shut and per perforation cells (flat physical
        indices, x fastest), WI, z."""
        return [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items() if k not in ("ijk", "axis")}
                for w in self.wells]
