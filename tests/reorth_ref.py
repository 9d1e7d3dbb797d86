"""One Gram-Schmidt step of the outer FGMRES with the optional second pass (tp_options.ksp_reorth) in numpy: the
reference of the GPU kernels behind tp_vec_orth_step and of tp_fgmres with ksp_reorth on.

    first pass    h = V^T w ;  w <- w - V h ;  n1 = ||w||^2
    criterion     "always": refine.  "ifneeded": refine iff n1 < eta^2 (||h||^2 + n1) and ||h||^2, n1 are finite
                  (||h||^2 + n1 stands for ||w||^2 of the vector that came in: ||w'|| < eta ||w||)
    second pass   c = V^T w ;  w <- w - V c ;  h <- h + c ;  n2 = ||w||^2

`dot` may be replaced as in tests/bcgs_ref.py (the sums taken in reversed order measure how far two legitimate summation orders
drive the results apart).  fgmres_ref is right-preconditioned FGMRES from x0 = 0 over this step, one cycle (no restart), with
the stopping rules of the GPU loop: recurrence residual <= max(rtol ||b||, atol), happy breakdown, non-finite residual.
"""
import numpy as np

from bcgs_ref import dot_forward, dot_reversed  # noqa: F401  (re-exported: the tests take both from here)

ETA = 2.0**-0.5
MODES = ("never", "ifneeded", "always")


def criterion(h, n1, eta):
    """The device's decision for "ifneeded" from the first pass's sums alone (no division)."""
    hh = float(np.sum(np.asarray(h, dtype=float)**2))
    return bool(np.isfinite(hh) and np.isfinite(n1) and n1 < eta*eta*(hh + n1))


def orth_step(V, w, mode="never", eta=ETA, dot=None):
    """V: sequence of k vectors, w: one vector of the same shape.  Returns (h, norm2, refined, w_out); w is not modified."""
    assert mode in MODES
    dot = dot or dot_forward
    k = len(V)
    h = np.array([dot(V[i], w) for i in range(k)])
    w = w - sum(h[i]*V[i] for i in range(k))
    n = dot(w, w)
    refined = mode == "always" or (mode == "ifneeded" and criterion(h, n, eta))
    if refined:
        c = np.array([dot(V[i], w) for i in range(k)])
        w = w - sum(c[i]*V[i] for i in range(k))
        h = h + c
        n = dot(w, w)
    return h, n, refined, w


def orth_figure(V, w):
    """max_i |<V_i, q>| with q = w / ||w||: how far the orthogonalised vector is from orthogonal to the basis."""
    q = w/np.sqrt(dot_forward(w, w))
    return max(abs(dot_forward(V[i], q)) for i in range(len(V)))


# ---- the near-dependent inputs of the step tests (tests/test_reorth_host.py on the reference, tests/test_gpu_reorth.py on the GPU) --
# (name, case builder in tests/cases.py, its arguments): a 2-D two-phase grid with fewer cells than one workgroup and a 3-D one
# whose owned count is no multiple of 256 * 8 entries (active tail lanes)
SHAPES = {"g2d": ("c3_spe10_2d", dict(Nx=7, Ny=9, nphase=2)), "g3d": ("c4_spe10_3d", dict(Nx=5, Ny=6, Nz=13, nphase=2))}
# internal vector shapes (fields, n2, n1, n0) of those grids
VSHAPE = {"g2d": (3, 1, 9, 7), "g3d": (3, 6, 5, 13)}
KS = (1, 4, 5, 17)              # straddle the 4-vector load batch of the kernels
DELTAS = (1e-8, 1e-4)


def near_dependent(shape, k, delta, seed=11):
    """V = k orthonormal vectors, w = V a + delta u with u orthogonal to V and ||a|| = ||u|| = 1.  The k + 1 directions are a
    seeded Gaussian matrix orthonormalised by Gram-Schmidt applied twice per column, with elementwise numpy operations and
    numpy's own sums only (no BLAS, no LAPACK): the same bits on every machine."""
    vs = VSHAPE[shape]
    n = int(np.prod(vs))
    rng = np.random.default_rng(seed + 1000*k + n)
    g = rng.standard_normal((k + 1, n))
    a = rng.standard_normal(k)
    a /= np.sqrt(dot_forward(a, a))
    q = []
    for i in range(k + 1):
        v = g[i]
        for _ in range(2):
            for p in q:
                v = v - dot_forward(p, v)*p
        q.append(v/np.sqrt(dot_forward(v, v)))
    w = delta*q[k]
    for i in range(k):
        w = w + a[i]*q[i]
    return [q[i].reshape(vs) for i in range(k)], w.reshape(vs)


# Measured on the CPU with this file alone (tests/test_reorth_host.py re-measures and checks them; profiles/reorth_parity.txt),
# over both shapes and every k of KS:
#  - orthogonality figure of the reference after one pass and after two, per delta: the largest (one pass: the smallest too).
#    One pass leaves ~ eps / delta; two passes leave ~ eps whatever delta is
#  - summation-order floor of the step: largest deviation between the forward and the reversed sums over all modes, of the
#    coefficients (max |dh| / ||h||) and of the final ||w||^2 (relative); the tolerance of the GPU comparison is 10 x the floor
#    (the GPU sums in a third order), per delta since the floor of ||w||^2 scales like eps / delta
ONE_PASS_FIGURE = {1e-8: (1.796e-11, 2.324e-08), 1e-4: (6.085e-15, 2.162e-12)}      # (smallest, largest); eps / delta = 2.2e-8, 2.2e-12
TWO_PASS_FIGURE = {1e-8: 3.470e-17, 1e-4: 5.205e-17}                                # largest
STEP_FLOOR = {1e-8: 3.59e-9, 1e-4: 1.63e-13}              # (measured 3.586e-9 at g2d, k = 17 and 1.626e-13 at g2d, k = 17)
STEP_TOL = {1e-8: 3.59e-8, 1e-4: 1.63e-12}
SEPARATION = 1e4                # two passes beat one by at least this factor at delta = 1e-8


def step_floor(shape, k, delta):
    """Largest deviation between the forward and the reversed sums of one step, over the three modes."""
    V, w = near_dependent(shape, k, delta)
    dev = 0.0
    for mode in MODES:
        hf, nf, rf, _ = orth_step(V, w, mode)
        hr, nr, rr, _ = orth_step(V, w, mode, dot=dot_reversed)
        assert rf == rr
        dev = max(dev, float(np.max(np.abs(hf - hr))/np.sqrt(np.sum(hf*hf))), abs(nf - nr)/nf)
    return dev


# ---- FGMRES over the step -----------------------------------------------------------------------------------------------------
def fgmres_ref(matvec, pc, b, rtol=1e-7, atol=1e-50, maxit=200, mode="never", eta=ETA, dot=None, info=None):
    """Returns (x, its, reason, hist) with hist[0] = ||b|| and hist[i] = the recurrence residual after iteration i.  info, when
    given, receives the Hessenberg columns before the rotations (hcol[j] = the j + 1 coefficients and ||w||) and, per iteration,
    whether the second pass ran (fired) and the margin n1 / (eta^2 (||h||^2 + n1)) of the "ifneeded" criterion."""
    dot = dot or dot_forward
    info = {} if info is None else info
    info.update(hcol=[], fired=[], margin=[])
    x = np.zeros_like(b)
    bb = dot(b, b)
    if not np.isfinite(bb):
        return x, 0, -9, [bb]
    beta = np.sqrt(bb)
    hist = [beta]
    if beta == 0.0:
        return x, 0, 2, hist
    tol = max(rtol*beta, atol)
    V, Z = [b/beta], []
    H = np.zeros((maxit + 1, maxit))
    cs, sn, g = np.zeros(maxit), np.zeros(maxit), np.zeros(maxit + 1)
    g[0] = beta
    its, reason = 0, -3
    for j in range(maxit):
        Z.append(pc(V[j]))
        w = matvec(Z[j])
        if mode == "ifneeded":         # (the margin of the criterion, from a first pass of its own)
            h1, n1, _, _ = orth_step(V, w, "never", dot=dot)
            info["margin"].append(n1/(eta*eta*(float(np.sum(h1**2)) + n1)))
        h, n2, fired, w = orth_step(V, w, mode, eta, dot)
        hn = np.sqrt(n2)
        info["hcol"].append(np.append(h, hn))
        info["fired"].append(fired)
        H[:j + 1, j] = h
        H[j + 1, j] = hn
        for i in range(j):
            t = cs[i]*H[i, j] + sn[i]*H[i + 1, j]
            H[i + 1, j] = -sn[i]*H[i, j] + cs[i]*H[i + 1, j]
            H[i, j] = t
        d = np.hypot(H[j, j], H[j + 1, j])
        cs[j], sn[j] = H[j, j]/d, H[j + 1, j]/d
        H[j, j], H[j + 1, j] = d, 0.0
        g[j + 1] = -sn[j]*g[j]
        g[j] = cs[j]*g[j]
        its = j + 1
        res = abs(g[j + 1])
        hist.append(res)
        if not np.isfinite(res) or res <= tol or hn == 0.0:
            reason = 2 if np.isfinite(res) else -9
            break
        V.append(w/hn)
    y = np.linalg.solve(np.triu(H[:its, :its]), g[:its]) if its and reason != -9 else np.zeros(its)
    for i in range(its):
        x = x + y[i]*Z[i]
    return x, its, reason, hist


# Summation-order floor of fgmres_ref on the systems of bcgs_ref.PARITY (fgmres_floor below, largest over all of them and over
# "always" and "ifneeded": c4_cpr) and the tolerance of the GPU comparison, 10 x the floor (profiles/reorth_parity.txt)
FGMRES_FLOOR = 4.32e-12
FGMRES_TOL = 4.4e-11


def solve_ref(o, J, b, mode, dot=None, info=None, **kw):
    """fgmres_ref on a system of tests/bcgs_ref.py (oracle_problem): the oracle's SpMV and two-stage preconditioner."""
    import oracle.linalg as la
    import bcgs_ref as R
    kw.setdefault("rtol", R.RTOL)
    return fgmres_ref(lambda v: la.spmv_block(J, v), o.pc.apply, b, mode=mode, dot=dot, info=info, **kw)


def fgmres_floor(o, J, b, mode, nhist=6):
    """Largest relative deviation between two runs of fgmres_ref that differ only in the order of their sums: over the first
    min(its, nhist) residual norms, the Hessenberg columns of those iterations (max |d| / ||column||) and the final x (rel2).
    Returns (floor, forward result, reversed result, forward info)."""
    fi, ri = {}, {}
    fw = solve_ref(o, J, b, mode, info=fi)
    rv = solve_ref(o, J, b, mode, dot=dot_reversed, info=ri)
    n = min(fw[1], rv[1], nhist)
    dev = [abs(fw[3][i] - rv[3][i])/fw[3][i] for i in range(1, n + 1)]
    dev += [float(np.max(np.abs(a - c))/np.linalg.norm(a)) for a, c in zip(fi["hcol"][:n], ri["hcol"][:n])]
    dev.append(float(np.linalg.norm((fw[0] - rv[0]).ravel())/np.linalg.norm(fw[0].ravel())))
    return max(dev), fw, rv, fi
