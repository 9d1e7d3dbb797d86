"""Reference of the fp32 factor stream (tp_options.ilu_single) for the tests: oracle.linalg.TiledILU0 with the solve written in
the DEVICE's form on the three arrays the device stores, each rounded to float32 (round to nearest):

    forward   B_cm = fl32(A_cm D~_m^-1)         y_c = r_c - sum_lower B_cm y_m
    backward  C_cm = fl32(D~_c^-1 A_cm)         x_c = fl32(D~_c^-1) y_c - sum_upper C_cm x_m

The factorisation itself is TiledILU0.factor, unchanged: float64 with the unrounded D~^-1 in the recurrence.  Vectors and
accumulation are float64.  Not a test module."""
import numpy as np

from oracle.linalg import TiledILU0


class SingleILU0(TiledILU0):
    def __init__(self, shape, tile, slabs=None, rounding=True):
        super().__init__(shape, tile, slabs)
        self.rounding = rounding
        self._for = None

    def _fl(self, a):
        return a.astype(np.float32).astype(np.float64) if self.rounding else a

    def _stored(self):
        """(B[3], C[3], Dr): what the device writes to its chunks, zero where the neighbour lies outside the tile."""
        if self._for is self.Dinv:
            return self._arrays
        Jf, Dinv = self.J, self.Dinv
        b, n = Jf.shape[1], Jf.shape[3]
        cells = np.arange(n)
        Bm, Cm = [], []
        for a in range(3):
            lo = cells[self.has_lo[a]]
            B = np.zeros((b, b, n))
            B[:, :, lo] = np.einsum("ijn,jkn->ikn", Jf[1 + 2*a][:, :, lo], Dinv[:, :, lo - self.strides[a]])
            Bm.append(self._fl(B))
            hi = cells[self.has_hi[a]]
            Cc = np.zeros((b, b, n))
            Cc[:, :, hi] = np.einsum("ijn,jkn->ikn", Dinv[:, :, hi], Jf[2 + 2*a][:, :, hi])
            Cm.append(self._fl(Cc))
        self._arrays = (Bm, Cm, self._fl(Dinv))
        self._for = self.Dinv
        return self._arrays

    def solve(self, r):
        Bm, Cm, Dr = self._stored()
        b, n = self.J.shape[1], self.J.shape[3]
        rf = r.reshape(b, n)
        y = np.zeros((b, n))
        for s in range(self.nlev):
            c = self.cells_at[s]
            t = rf[:, c].copy()
            for a in range(3):
                m = self.has_lo[a][c]
                cc = c[m]
                if len(cc):
                    t[:, m] -= np.einsum("ijn,jn->in", Bm[a][:, :, cc], y[:, cc - self.strides[a]])
            y[:, c] = t
        x = np.zeros((b, n))
        for s in range(self.nlev - 1, -1, -1):
            c = self.cells_at[s]
            t = np.einsum("ijn,jn->in", Dr[:, :, c], y[:, c])
            for a in range(3):
                m = self.has_hi[a][c]
                cc = c[m]
                if len(cc):
                    t[:, m] -= np.einsum("ijn,jn->in", Cm[a][:, :, cc], x[:, cc + self.strides[a]])
            x[:, c] = t
        return x.reshape(r.shape)


def swap_into(oracle_engine, rounding=True):
    """Replace the stage-2 solver of an OracleEngine's preconditioner (before its setup) by SingleILU0 on the same tiles."""
    pc = oracle_engine.pc
    pc.ilu = SingleILU0(oracle_engine.prob.shape, oracle_engine.opts["ilu_tile"], pc.slabs, rounding=rounding)
    return pc.ilu
