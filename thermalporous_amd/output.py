"""Field output for ParaView: the reference writes `results/pressure.pvd`, `temperature.pvd` and `saturation_o.pvd`
through Firedrake's `File` at t = 0 and every `n_save` time steps (thermalmodel.py:113-133, 303-322).  Here each
`File` is a PVD collection of VTK ImageData (`.vti`) pieces -- the grids are structured boxes, cell data, raw
little-endian float64 base64-inlined -- written with the standard library only.  A geo with spacing (geo.set_spacing) has
cells of unequal width, which ImageData cannot describe: its pieces are VTK RectilinearGrid (`.vtr`) files that carry the true
edge coordinates of every axis."""
import base64
import os
import struct

import numpy as np


class File():
    def __init__(self, path):
        self.path = path
        self.base = os.path.splitext(path)[0]
        self.entries = []          # (time, vti file name)
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)

    def write(self, name, values, geo, time=0.0):
        """values: one double per cell, x fastest then y then z (the model's field-major order)."""
        nx, ny, nz = geo.Nx, geo.Ny, getattr(geo, "Nz", 1)
        dx, dy, dz = geo.Dx, geo.Dy, getattr(geo, "Dz", 1.0)
        a = np.ascontiguousarray(np.asarray(values, dtype="<f8").reshape(-1))
        if a.size != nx*ny*nz:
            raise ValueError("field has %d values for a %dx%dx%d grid" % (a.size, nx, ny, nz))
        payload = _b64(a)
        if getattr(geo, "graded", False):
            fn = "%s_%d.vtr" % (self.base, len(self.entries))
            self._write_vtr(fn, name, payload, geo, (nx, ny, nz))
        else:
            fn = "%s_%d.vti" % (self.base, len(self.entries))
            self._write_vti(fn, name, payload, (nx, ny, nz), (dx, dy, dz))
        self.entries.append((float(time), os.path.basename(fn)))
        with open(self.path, "w") as f:
            f.write('<?xml version="1.0"?>\n<VTKFile type="Collection" version="0.1" byte_order="LittleEndian">\n')
            f.write('  <Collection>\n')
            for t, e in self.entries:
                f.write('    <DataSet timestep="%r" part="0" file="%s"/>\n' % (t, e))
            f.write('  </Collection>\n</VTKFile>\n')

    @staticmethod
    def _write_vtr(fn, name, payload, geo, n):
        nx, ny, nz = n
        edges = list(geo.cell_edges())
        if len(edges) == 2:
            edges.append(np.array([0.0, 1.0]))          # 2-D: one layer of unit thickness, as the ImageData pieces have
        with open(fn, "w") as f:
            f.write('<?xml version="1.0"?>\n<VTKFile type="RectilinearGrid" version="0.1" byte_order="LittleEndian">\n')
            f.write('  <RectilinearGrid WholeExtent="0 %d 0 %d 0 %d">\n' % (nx, ny, nz))
            f.write('    <Piece Extent="0 %d 0 %d 0 %d">\n      <CellData Scalars="%s">\n' % (nx, ny, nz, name))
            f.write('        <DataArray type="Float64" Name="%s" format="binary">%s</DataArray>\n' % (name, payload))
            f.write('      </CellData>\n      <Coordinates>\n')
            for ax, e in zip("xyz", edges):
                f.write('        <DataArray type="Float64" Name="%s" format="binary">%s</DataArray>\n' % (ax, _b64(e)))
            f.write('      </Coordinates>\n    </Piece>\n  </RectilinearGrid>\n</VTKFile>\n')

    @staticmethod
    def _write_vti(fn, name, payload, n, d):
        nx, ny, nz = n
        dx, dy, dz = d
        with open(fn, "w") as f:
            f.write('<?xml version="1.0"?>\n<VTKFile type="ImageData" version="0.1" byte_order="LittleEndian">\n')
            f.write('  <ImageData WholeExtent="0 %d 0 %d 0 %d" Origin="0 0 0" Spacing="%r %r %r">\n'
                    % (nx, ny, nz, dx, dy, dz))
            f.write('    <Piece Extent="0 %d 0 %d 0 %d">\n      <CellData Scalars="%s">\n' % (nx, ny, nz, name))
            f.write('        <DataArray type="Float64" Name="%s" format="binary">%s</DataArray>\n' % (name, payload))
            f.write('      </CellData>\n    </Piece>\n  </ImageData>\n</VTKFile>\n')


def _b64(a):
    """One inline binary DataArray: uint32 byte count, then the doubles, base64."""
    raw = np.ascontiguousarray(np.asarray(a, dtype="<f8").reshape(-1)).tobytes()
    return base64.b64encode(struct.pack("<I", len(raw)) + raw).decode()


def _unb64(text):
    blob = base64.b64decode(text.strip())
    n = struct.unpack("<I", blob[:4])[0]
    return np.frombuffer(blob[4:4 + n], dtype="<f8")


def read_vti(path):
    """(name, values) of the single cell array of a file written above (used by the tests)."""
    import xml.etree.ElementTree as ET
    arr = ET.parse(path).getroot().find("ImageData/Piece/CellData/DataArray")
    blob = base64.b64decode(arr.text.strip())
    n = struct.unpack("<I", blob[:4])[0]
    return arr.get("Name"), np.frombuffer(blob[4:4 + n], dtype="<f8")


def read_vtr(path):
    """(name, values, (x, y, z)) of a RectilinearGrid piece written above: the single cell array and the edge coordinates."""
    import xml.etree.ElementTree as ET
    piece = ET.parse(path).getroot().find("RectilinearGrid/Piece")
    arr = piece.find("CellData/DataArray")
    coords = {c.get("Name"): _unb64(c.text) for c in piece.findall("Coordinates/DataArray")}
    return arr.get("Name"), _unb64(arr.text), (coords["x"], coords["y"], coords["z"])
