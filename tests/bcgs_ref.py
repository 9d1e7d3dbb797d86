"""Right-preconditioned (flexible) BiCGStab from x0 = 0 in numpy: the reference of the GPU solver tp_bcgs
(thermalporous_amd/csrc/tp_bcgs.hip), with the same latches and reason codes.

    r = b; r^ = b; rho = (b,b); tol = max(rtol ||b||, atol)
    repeat i = 1..maxit:
      rho == 0 -> -5;  p = r + beta (p - omega v)   (beta = (rho/rho_old)(alpha/omega); first iteration: p = r)
      p^ = M p;  v = J p^;  (r^,v) == 0 -> -5;  alpha = rho / (r^,v)
      s = r - alpha v;  ||s|| <= tol: half-step exit, omega := 0
      s^ = M s;  t = J s^;  omega = (t,s)/(t,t)    (0 if (t,t) == 0 or on the half-step exit)
      x += alpha p^ + omega s^;  r = s - omega t;  stop on ||r|| <= tol

Reasons (KSP numbering): 2 converged (b = 0: with zero iterations), -3 maxit reached, -5 breakdown (rho == 0, (r^,v) == 0, or
omega == 0 with r still above the tolerance, where the next beta would divide by zero), -9 a sum that is not finite.  A
breakdown or NaN found inside an iteration leaves x and r as they were before it and does not count the iteration.

`dot` may be replaced (the GPU tests run it a second time with the sums taken in reversed order to measure how far two
legitimate summation orders drive the iteration apart).  info, when given, receives the ||s|| history and the half-step flag.
"""
import numpy as np


def dot_forward(u, v):
    return float(np.sum(u.ravel()*v.ravel()))          # (numpy's pairwise sum: no BLAS, the same grouping on every machine)


def dot_reversed(u, v):
    return float(np.sum((u.ravel()*v.ravel())[::-1]))


def bcgs_ref(matvec, pc, b, rtol=1e-7, atol=1e-50, maxit=200, dot=None, info=None):
    """Returns (x, its, reason, hist) with hist[0] = ||b|| and hist[i] = ||r|| after iteration i."""
    dot = dot or dot_forward
    info = {} if info is None else info
    info.update(snorm=[], half=False)
    x = np.zeros_like(b)
    rho = dot(b, b)
    if not np.isfinite(rho):
        return x, 0, -9, [np.sqrt(rho) if rho == rho and rho > 0 else rho]
    bnorm = np.sqrt(rho)
    hist = [bnorm]
    if bnorm == 0.0:
        return x, 0, 2, hist
    tol = max(rtol*bnorm, atol)
    r = b.copy()
    rh = b.copy()
    p = v = None
    alpha = omega = beta = 0.0
    its = 0
    while True:
        # (beta was formed at the end of the previous iteration; 0 marks the first one)
        p = r.copy() if beta == 0.0 else r + beta*(p - omega*v)
        ph = pc(p)
        v = matvec(ph)
        rv = dot(rh, v)
        if not np.isfinite(rv):
            return x, its, -9, hist
        if rv == 0.0:
            return x, its, -5, hist
        alpha = rho/rv
        if not np.isfinite(alpha):
            return x, its, -9, hist
        s = r - alpha*v
        ss = dot(s, s)
        if not np.isfinite(ss):
            return x, its, -9, hist
        half = bool(np.sqrt(ss) <= tol)
        info["snorm"].append(np.sqrt(ss))
        sh = pc(s)
        t = matvec(sh)
        ts, tt = dot(t, s), dot(t, t)
        if not (np.isfinite(ts) and np.isfinite(tt)):
            return x, its, -9, hist
        omega = 0.0 if (half or tt == 0.0) else ts/tt
        if not np.isfinite(omega):
            return x, its, -9, hist
        x = x + alpha*ph
        if omega != 0.0:
            x = x + omega*sh
            r = s - omega*t
        else:
            r = s
        rho_new, rr = dot(rh, r), dot(r, r)
        its += 1
        if not (np.isfinite(rho_new) and np.isfinite(rr)):
            return x, its - 1, -9, hist
        hist.append(np.sqrt(rr))
        if np.sqrt(rr) <= tol:
            info["half"] = half
            return x, its, 2, hist
        if its >= maxit:
            return x, its, -3, hist
        if rho_new == 0.0 or omega == 0.0:
            return x, its, -5, hist
        beta = (rho_new/rho)*(alpha/omega)
        if not np.isfinite(beta):
            return x, its - 1, -9, hist          # (reported like every other NaN: the solver's count excludes the iteration that found it)
        rho = rho_new


# ---- the linear systems the GPU tests solve (tests/test_gpu_bcgs.py) and the CPU checks on them (tests/test_bcgs_host.py) ------
T2D = (1 << 30, 64, 1)
RTOL = 1e-7
DT = 8640.0


def _shapes():
    import cases
    return {"c1": (cases.c1_homogeneous, dict(N=12, nphase=1)), "c3": (cases.c3_spe10_2d, dict(Nx=14, Ny=19, nphase=2)),
            "c4": (cases.c4_spe10_3d, dict(Nx=7, Ny=13, Nz=9, nphase=2))}


# (name, shape, engine options, dt, seed of the perturbed state): every preconditioner kind on the shapes it exists for.  dt and
# seed were chosen on the CPU, from the reference alone: the first candidates whose reference history stays a factor 2 away
# from the tolerance at the steps around its stop, in both summation orders (tests/test_bcgs_host.py checks every one of them).
PARITY = [("c1_cpr", "c1", dict(pc="cpr", ilu_tile=T2D), 8640.0, 5), ("c1_fieldsplit_cd", "c1", dict(pc="fieldsplit_cd", ilu_tile=T2D), 86.4, 2),
          ("c1_bilu", "c1", dict(pc="bilu", ilu_tile=T2D), 8640.0, 3),
          ("c3_cpr", "c3", dict(pc="cpr", ilu_tile=T2D), 864.0, 4), ("c3_cptr", "c3", dict(pc="cptr", ilu_tile=T2D), 864.0, 8),
          ("c3_cptramg_QI", "c3", dict(pc="cptramg", decoup="QI", ilu_tile=T2D), 86.4, 8), ("c3_bilu", "c3", dict(pc="bilu", ilu_tile=T2D), 86.4, 2),
          ("c4_cpr", "c4", dict(pc="cpr"), 864.0, 7), ("c4_cptr", "c4", dict(pc="cptr"), 86.4, 3),
          ("c4_cptramg_QI", "c4", dict(pc="cptramg", decoup="QI"), 864.0, 5), ("c4_bilu", "c4", dict(pc="bilu"), 0.864, 7),
          # stage-2 tiles of one plane of the slab axis: the same preconditioner however the 13 planes are cut into slabs
          ("c4_cptr_planes", "c4", dict(pc="cptr", ilu_tile=(1 << 30, 16, 1), amg_gather_cells=-1), 86.4, 3)]
# Summation-order floor of these inputs (summation_floor below, largest over all cases: c4_cptramg_QI) and the tolerance of
# the GPU comparison, 10 x the floor: the GPU sums in a third order (profiles/bcgs_parity.txt)
PARITY_FLOOR = 7.13e-6
PARITY_TOL = 7.2e-5
# the half-step test: b = J M e for a smooth e on c4 / cptr at this time step and tolerance (the reference leaves through the
# half step after 4 iterations, clear of the tolerance)
HALF = ("c4", dict(pc="cptr"), 864.0, 3, 1e-2)


def smooth_rhs(o, J):
    import oracle.linalg as la
    sh = (J.shape[1],) + J.shape[3:]
    z, y, x = np.meshgrid(*[np.linspace(0, 1, n) for n in sh[1:]], indexing="ij")
    e = np.array([(1.0 + 0.5*f)*np.cos(np.pi*x)*np.cos(np.pi*y)*np.cos(np.pi*z) + 0.3 for f in range(sh[0])])
    return la.spmv_block(J, o.pc.apply(e))


def oracle_problem(shape, opts, seed=5, amp=0.3, dt=DT):
    """The oracle engine at a perturbed state with its preconditioner set up: (spec, u0, u, engine, J, F = Newton right-hand side)."""
    from oracle.engine import OracleEngine
    import cases
    builder, kw = _shapes()[shape]
    spec, u0, *_ = builder(**kw)
    o = OracleEngine(spec, opts)
    u = cases.perturbed_state(spec, seed=seed, amp=amp)
    o.set_old(u0)
    o.set_dt(dt)
    o.set_state(u)
    schur = opts["pc"] in ("cptr", "fieldsplit_cd")
    out = o.jacobian(want_schur=schur)
    J, Sm = out if schur else (out, None)
    o.pc.setup(J, Sm)
    F = o.residual()
    return spec, u0, u, o, J, F


def solve_ref(o, J, b, dot=None, info=None, **kw):
    import oracle.linalg as la
    kw.setdefault("rtol", RTOL)
    return bcgs_ref(lambda v: la.spmv_block(J, v), o.pc.apply, b, dot=dot, info=info, **kw)


def clear_of_tolerance(hist, snorm, tol):
    """The residual history stays a factor 2 away from tol at the steps around its stop: the last two ||r|| and the ||s|| of the
    last two iterations (a half-step exit is a stop too)."""
    around = list(hist[1:][-2:]) + list(snorm[-2:])
    return not any(tol/2 <= r <= 2*tol for r in around)


def summation_floor(o, J, b, nhist=6):
    """Largest relative deviation between two runs of the reference that differ only in the order of their sums: over the first
    min(its, nhist) residual norms, and the final x (rel2).  Returns (floor, forward result, reversed result, info)."""
    info = {}
    fw = solve_ref(o, J, b, info=info)
    rv = solve_ref(o, J, b, dot=dot_reversed)
    n = min(fw[1], rv[1], nhist)
    dev = [abs(fw[3][i] - rv[3][i])/fw[3][i] for i in range(1, n + 1)]
    dev.append(float(np.linalg.norm((fw[0] - rv[0]).ravel())/np.linalg.norm(fw[0].ravel())))
    return max(dev), fw, rv, info
