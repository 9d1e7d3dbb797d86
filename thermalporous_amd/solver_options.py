"""PETSc-style ``solver_parameters`` of the reference -> options of the compute engine.

The reference configures its whole linear/nonlinear stack through PETSc option dicts
(singlephase.py:289-354,410-439; twophase.py:416-433,531-597,929-997).  The hot path honours the
subset that selects the solvers it implements and rejects everything else loudly -- every key is either
CONSUMED (and its value checked against what is implemented), purely cosmetic (monitors/views), or an error:

  snes_type newtonls, snes_linesearch_type basic (Firedrake's default) | bt: Armijo backtracking (engine key linesearch = "bt")
     with snes_linesearch_order 2|3 (default 3, PETSc's), snes_linesearch_alpha, snes_linesearch_max_it,
     snes_linesearch_maxstep, snes_linesearch_minlambda (absolute here) -> ls_order, ls_alpha, ls_max_it, ls_maxstep,
     ls_minlambda; any of them without bt raises.  l2 and cp are not implemented
  ksp_type fgmres|gmres (right preconditioning), ksp_rtol/atol/max_it, ksp_gmres_restart
  ksp_gmres_cgs_refinement_type refine_never (PETSc's and this build's default) | refine_ifneeded | refine_always -> engine key
     ksp_reorth = "never" | "ifneeded" | "always" (a second classical Gram-Schmidt pass, decided on the device; eta of the
     ifneeded rule is the build key ksp_reorth_eta).  FGMRES with fp64 bases only.  ksp_gmres_modifiedgramschmidt is not consumed
  ksp_type fbcgs | bcgs + ksp_pc_side right: right-preconditioned BiCGStab (engine key ksp = "bcgs"); ksp_gmres_restart is
     consumed and has no effect on it
  pc_type composite, pc_composite_type multiplicative, pc_composite_pcs "python,bjacobi"
     also "bjacobi,X" | "bjacobi,X,bjacobi" | "X,bjacobi,X", X = python or fieldsplit (blanks and one trailing comma ignored): the
     engine key pc_order = "IS" | "ISI" | "SIS"; the k-th entry's keys carry sub_k_, a repeated entry must be configured identically
     with the build key pc_ctr: True in the same dict, one more trailing "fieldsplit" entry whose pc_fieldsplit_0_fields is "1": the
     temperature-only stage of the reference's cprctr composites (additive, fieldsplit_0 = one V-cycle, fieldsplit_1 = gmres /
     ksp_max_it 0 / pc_type none on the remaining fields); without the key that entry is refused by name
     sub_0_pc_python_type  ...CPRStage1PC | ...CPTRStage1PC   sub_0_cpr_decoup  No|QI|TI
     sub_0_cpr_stage1*     boomeramg V-cycle / fieldsplit-schur with ConvDiffSchurTwoPhasesPC
  pc_fieldsplit_schur_fact_type FULL | lower | upper | diag (any letter case, as PETSc) under the prefix of the Schur split on (p,T)
     -- "", sub_0_fieldsplit_0_ or sub_0_cpr_stage1_ -> engine key schur_fact = "full" | "lower" | "upper" | "diag"; with diag,
     pc_fieldsplit_schur_scale under the same prefix -> schur_scale (PETSc's default -1).  The scale with another fact type is a
     ValueError (PETSc would ignore it), as is a fact type or scale given both as build key and as PETSc key with different values
     sub_1_sub_pc_type ilu, sub_1_sub_pc_factor_levels 0, sub_1_pc_bjacobi_blocks
  inner solve of the stage-1 PRESSURE solver K(A00) (pc_cptramg*: of the (p,T) system solver), under that solver's prefix
  (_take_inner): pc_hypre_boomeramg_max_iter k | ksp_type richardson, ksp_max_it k | ksp_type fgmres (gmres + ksp_pc_side
  right), ksp_max_it k <= 32, ksp_rtol, ksp_atol -- also spelled pc_type ksp + ksp_<the same keys> -> s1_ksp, s1_max_it,
  s1_rtol, s1_atol.  The Schur / temperature solvers stay one V-cycle.

  snes_ksp_ew (flag): Eisenstat-Walker inexact Newton, the tolerance of every linear solve chosen from the nonlinear residuals
     (engine key ksp_ew = 1 | 2, True = 2), with snes_ksp_ew_version 1|2 (default 2; 3 is not implemented), snes_ksp_ew_rtol0,
     _rtolmax, _gamma, _alpha, _alpha2, _threshold (PETSc's defaults and ranges) -> ew_rtol0 ... ew_threshold; any of them without
     the flag raises.  Unlike PETSc the configured ksp_rtol stays as the tolerance's floor; ksp_rtol > rtolmax is a ValueError

Defaults the reference inherits silently from Firedrake/PETSc are fixed here explicitly
(SURVEY.md 8c): ksp_rtol 1e-7 (Firedrake), snes_rtol 1e-8, snes_atol 1e-50, snes_stol 1e-8,
ksp_atol 1e-50; an inner fgmres without ksp_rtol/ksp_atol gets PETSc's own KSP defaults, 1e-5 and 1e-50.
Build-specific tuning keys (not PETSc): amg_omega, amg_nu, amg_min_cells, ilu_tile, s1_ksp, s1_max_it, s1_rtol, s1_atol, linesearch,
ksp_reorth, ksp_reorth_eta, pc_order, pc_ctr, schur_fact, schur_scale, ksp_ew, ew_rtol0, ew_rtolmax, ew_gamma, ew_alpha, ew_alpha2, ew_threshold, ls_order, ls_alpha, ls_max_it, ls_maxstep, ls_minlambda, ls_max_change (per-field cap on the change per Newton iteration).  Two-phase string presets are layered on plain Newton-Krylov, not on the reference's
experimental FAS nonlinear preconditioner (twophase.py:927; needs mesh hierarchies + MUMPS).
"""

# keys that only print / name the matrix type: no effect on the arithmetic
_IGNORED = {"snes_monitor", "snes_converged_reason", "ksp_converged_reason", "ksp_view", "snes_view", "ksp_monitor",
            "ksp_monitor_residuals"}      # (ksp_monitor_residuals is honoured by ThermalModel.init_solver, like the reference)

# every PETSc key the hot path CONSUMES (checked against the value it implements) -- anything else raises
_VCYCLE_SUFFIXES = {"ksp_type": "preonly", "pc_type": "hypre", "pc_hypre_type": "boomeramg",
                    "pc_hypre_boomeramg_max_iter": 1}


_SCHUR_WHY = ("an iterative solver on the Schur split is not implemented: PETSc would iterate on the TRUE Schur complement "
              "A11 - A10 K(A00) A01, which needs nested A00 solves in every mat-vec; only the pressure solver K(A00) (and "
              "the (p,T) system solver of pc_cptramg) can be an inner iteration")
_ADDITIVE_WHY = ("an iterative solver on the temperature block of the additive split is not implemented: only the pressure "
                 "solver K(A00) is wired to the inner iteration")
_CTR_WHY = ("an iterative solver in the composite's temperature-only stage is not implemented: that stage (pc_ctr) is always one "
            "V-cycle on A_TT; only the pressure solver K(A00) of an S stage is wired to the inner iteration")
_CGS_REFINE = {"refine_never": "never", "refine_ifneeded": "ifneeded", "refine_always": "always"}
_S1_MAXK = 32              # GMRES(k) without restart: k basis vectors of the stage-1 block are stored


_STAGE_OF = {"python": "S", "fieldsplit": "S", "bjacobi": "I"}
_ORDERS = ("SI", "IS", "ISI", "SIS")
_MISSING = object()


def _take(sp, used, key, allowed=None, default=None):
    """Consume `key`; `allowed` = the values the hot path implements."""
    if key not in sp:
        return default
    v = sp[key]
    if allowed is not None and v not in allowed:
        raise NotImplementedError("%s = %r is not implemented on the hot path (supported: %s)"
                                  % (key, v, ", ".join(repr(a) for a in allowed)))
    used.add(key)
    return v


def _set_checked(o, key, value, given, what, said, norm=lambda v: v):
    """o[key] = value, read from the PETSc spelling.  ``given``: the dict as the caller wrote it, whose build key ``key`` must agree
    (compared through ``norm``); what, said: what the message calls the option, and the two spellings side by side."""
    if key in given and norm(o[key]) != norm(value):
        raise ValueError("%s is configured twice and differently: %s" % (what, said))
    o[key] = value


def _take_zero_split(sp, used, prefix):
    """``<prefix>pc_fieldsplit_type additive`` whose second split returns zero: ``<prefix>fieldsplit_1_`` = gmres, ksp_max_it 0,
    pc_type none.  Consumes the four keys; whether all of them are there with these values."""
    _take(sp, used, prefix + "pc_fieldsplit_type", ("additive",))
    _take(sp, used, prefix + "fieldsplit_1_ksp_type", ("gmres",))
    _take(sp, used, prefix + "fieldsplit_1_pc_type", ("none",))
    return (prefix + "pc_fieldsplit_type" in used and prefix + "fieldsplit_1_ksp_type" in used
            and int(_take(sp, used, prefix + "fieldsplit_1_ksp_max_it", None, -1)) == 0 and prefix + "fieldsplit_1_pc_type" in used)


def _take_vcycle(sp, prefix, used, schur=False):
    """``<prefix>`` must configure exactly the reference's one-V-cycle solver (v_cycle dicts, singlephase.py:303-307,
    twophase.py:478-482); hypre tuning keys are not honoured and therefore rejected.  schur: the prefix is (inside) the
    Schur split (or, "additive", the temperature block of the additive split), where an inner iteration is rejected with the
    reason."""
    for suf, want in _VCYCLE_SUFFIXES.items():
        k = prefix + suf
        if k not in sp:
            if suf == "pc_hypre_boomeramg_max_iter":      # PETSc's default is already 1
                continue
            raise NotImplementedError("%s missing: the stage-1 solver must be one BoomerAMG V-cycle (v_cycle)" % k)
        if sp[k] != want:
            if schur and suf in ("ksp_type", "pc_hypre_boomeramg_max_iter"):
                raise NotImplementedError("%s = %r: %s" % (k, sp[k], {"additive": _ADDITIVE_WHY, "ctr": _CTR_WHY}.get(schur, _SCHUR_WHY)))
            raise NotImplementedError("%s = %r: only %r (one V-cycle per application)" % (k, sp[k], want))
        used.add(k)
    for k in sp:
        if k.startswith(prefix + "pc_hypre_") and k not in used:
            raise NotImplementedError("%s: hypre tuning options do not apply to this build's own AMG" % k)


def _set_inner(o, ksp, k, rtol=0.0, atol=0.0):
    new = dict(s1_ksp=ksp, s1_max_it=int(k), s1_rtol=float(rtol), s1_atol=float(atol))
    if o.get("s1_ksp", "preonly") != "preonly" and any(o[q] != v for q, v in new.items()):
        raise ValueError("the inner stage-1 solve is configured twice and differently: build keys %r, PETSc keys %r"
                         % ({q: o[q] for q in new}, new))
    o.update(new)


_SCHUR_FACTS = ("full", "lower", "upper", "diag")


def _take_schur_fact(sp, used, prefix, o, given):
    """``<prefix>pc_fieldsplit_schur_fact_type`` (FULL | lower | upper | diag in any letter case, as PETSc reads it) and
    ``<prefix>pc_fieldsplit_schur_scale`` -> the engine keys schur_fact and schur_scale.  Returns whether the fact-type key is there
    with one of the four values; the caller refuses the split otherwise.  ``given``: the dict as the caller got it, whose build
    keys schur_fact / schur_scale must agree with the PETSc spelling."""
    kf, ks = prefix + "pc_fieldsplit_schur_fact_type", prefix + "pc_fieldsplit_schur_scale"
    fact = str(sp.get(kf, "")).lower()
    if fact not in _SCHUR_FACTS:
        return False
    used.add(kf)
    _set_checked(o, "schur_fact", fact, given, "the Schur factorisation", "schur_fact = %r, %s = %r" % (o["schur_fact"], kf, sp[kf]))
    if ks in sp:
        scale = sp[ks]
        used.add(ks)
        if isinstance(scale, bool) or not isinstance(scale, (int, float)):
            raise ValueError("%s = %r: a number" % (ks, scale))
        if fact != "diag":
            raise ValueError("%s = %r with %s = %r: the scale belongs to the diag factorisation (PETSc would silently ignore it)"
                             % (ks, scale, kf, sp[kf]))
        _set_checked(o, "schur_scale", float(scale), given, "the Schur factorisation",
                     "schur_scale = %r, %s = %r" % (o["schur_scale"], ks, scale), norm=float)
    return True


def _take_inner(sp, prefix, used, o, ksp_default=None):
    """The V-cycle solver at ``<prefix>`` that may be an inner iteration: the stage-1 pressure solver K(A00), or the (p,T)
    system solver of pc_cptramg*.  A python stage-1 class holds a PC, not a KSP (preconditioners.py:633 of the reference), so
    PETSc itself wants ``<prefix>pc_type ksp`` with the solver keys under ``<prefix>ksp_``: both spellings are taken."""
    kp = prefix
    if sp.get(prefix + "pc_type") == "ksp":
        used.add(prefix + "pc_type")
        _take(sp, used, prefix + "ksp_type", ("preonly",))
        kp = prefix + "ksp_"
    ksp = sp.get(kp + "ksp_type", ksp_default if kp == prefix else None)    # (a PC handle has no ksp_type of its own)
    if ksp is None:
        raise NotImplementedError("%sksp_type missing: the stage-1 solver is a BoomerAMG V-cycle (v_cycle), alone or inside "
                                  "richardson / fgmres" % kp)
    if ksp not in ("preonly", "richardson", "fgmres", "gmres"):
        raise NotImplementedError("%sksp_type = %r: preonly, richardson or fgmres (gmres with ksp_pc_side right) around "
                                  "the V-cycle" % (kp, ksp))
    if kp + "ksp_type" in sp:
        used.add(kp + "ksp_type")
    for suf, want in (("pc_type", "hypre"), ("pc_hypre_type", "boomeramg")):
        if sp.get(kp + suf) != want:
            raise NotImplementedError("%s%s = %r: only %r (the build's own AMG V-cycle)" % (kp, suf, sp.get(kp + suf), want))
        used.add(kp + suf)
    m = sp.get(kp + "pc_hypre_boomeramg_max_iter", 1)
    if kp + "pc_hypre_boomeramg_max_iter" in sp:
        used.add(kp + "pc_hypre_boomeramg_max_iter")
    if int(m) != m or m < 1:
        raise ValueError("%spc_hypre_boomeramg_max_iter = %r: a count >= 1" % (kp, m))
    for k in sp:
        if k.startswith(kp + "pc_hypre_") and k not in used:
            raise NotImplementedError("%s: hypre tuning options do not apply to this build's own AMG" % k)
    if ksp == "preonly":
        if m > 1:                    # k V-cycles as a stationary iteration from x0 = 0
            _set_inner(o, "richardson", m)
        return
    if m != 1:
        raise NotImplementedError("%sksp_type %s around pc_hypre_boomeramg_max_iter %d: one V-cycle per inner iteration" % (kp, ksp, m))
    if kp + "ksp_max_it" not in sp:
        raise NotImplementedError("%sksp_max_it missing: the inner iteration count is fixed (PETSc's default of 10000 is not)" % kp)
    k = sp[kp + "ksp_max_it"]
    used.add(kp + "ksp_max_it")
    if int(k) != k or k < 1:
        raise ValueError("%sksp_max_it = %r: a count >= 1" % (kp, k))
    if ksp == "richardson":
        # exactly k V-cycles: ksp_rtol / ksp_atol are not consumed (they would be silently ignored, so they raise)
        _take(sp, used, kp + "ksp_norm_type", ("none",))
        _set_inner(o, "richardson", k)
        return
    side = _take(sp, used, kp + "ksp_pc_side", ("right",))
    if ksp == "gmres" and side is None:
        raise NotImplementedError("%sksp_type gmres without ksp_pc_side: PETSc would precondition from the LEFT; only "
                                  "right-preconditioned (F)GMRES is implemented (the reference sets ksp_pc_side right, "
                                  "singlephase.py:296)" % kp)
    if k > _S1_MAXK:
        raise NotImplementedError("%sksp_max_it = %d: the inner GMRES keeps its whole basis (no restart), at most %d iterations"
                                  % (kp, k, _S1_MAXK))
    restart = _take(sp, used, kp + "ksp_gmres_restart")
    if restart is not None and restart < k:
        raise NotImplementedError("%sksp_gmres_restart %d < ksp_max_it %d: the inner GMRES does not restart" % (kp, restart, k))
    rtol = _take(sp, used, kp + "ksp_rtol", None, 1e-5)          # PETSc's KSP defaults
    atol = _take(sp, used, kp + "ksp_atol", None, 1e-50)
    if rtol < 0 or atol < 0:
        raise ValueError("%sksp_rtol / ksp_atol must be >= 0" % kp)
    _set_inner(o, "fgmres", k, rtol, atol)


def _check_inner(o):
    """Validate s1_* however they were given (build keys or PETSc spelling), ilu_single against the stage-2 layout and
    amg_line_levels against what it excludes (the slab count is the engine's to check)."""
    from .engine import check_ilu_single_options, check_options
    check_ilu_single_options(o, NotImplementedError)      # (blocks of several tiles depend on the grid: resolve_ilu_options)
    check_options(o, exc=NotImplementedError)
    ksp, k = o["s1_ksp"], o["s1_max_it"]
    if ksp not in ("preonly", "richardson", "fgmres"):
        raise NotImplementedError("s1_ksp = %r: preonly, richardson or fgmres" % (ksp,))
    if ksp == "preonly":
        return
    if o["pc"] == "bilu":
        raise NotImplementedError("pc_bilu has no stage-1 solver: s1_ksp does not apply")
    if int(k) != k or k < 1:
        raise ValueError("s1_max_it = %r: a count >= 1" % (k,))
    if ksp == "fgmres" and k > _S1_MAXK:
        raise NotImplementedError("s1_max_it = %d: the inner GMRES keeps its whole basis (no restart), at most %d" % (k, _S1_MAXK))
    if o["s1_rtol"] < 0 or o["s1_atol"] < 0:
        raise ValueError("s1_rtol / s1_atol must be >= 0")


_EW_KEYS = (("snes_ksp_ew_rtol0", "ew_rtol0"), ("snes_ksp_ew_rtolmax", "ew_rtolmax"), ("snes_ksp_ew_gamma", "ew_gamma"),
            ("snes_ksp_ew_alpha", "ew_alpha"), ("snes_ksp_ew_alpha2", "ew_alpha2"), ("snes_ksp_ew_threshold", "ew_threshold"))


def _take_ew(sp, used, o, given):
    """snes_ksp_ew (a flag: None or True; False is off) and snes_ksp_ew_version / _rtol0 / _rtolmax / _gamma / _alpha / _alpha2 /
    _threshold -> ksp_ew and the ew_* keys.  A snes_ksp_ew_* key without the flag raises, as PETSc would silently ignore it; both
    spellings given and disagreeing is a ValueError."""
    from .engine import ew_version
    flag = None
    if "snes_ksp_ew" in sp:
        v = sp["snes_ksp_ew"]
        if not (v is None or isinstance(v, bool)):
            raise ValueError("snes_ksp_ew = %r: a flag (None or True), or False for off; the version is snes_ksp_ew_version" % (v,))
        flag = v is None or v
        used.add("snes_ksp_ew")
    sub_keys = [k for k in sp if k.startswith("snes_ksp_ew_")]
    if sub_keys and not flag:
        raise NotImplementedError("%s without snes_ksp_ew: the key belongs to the Eisenstat-Walker tolerances, which the flag "
                                  "snes_ksp_ew switches on (it would be silently ignored)" % sorted(sub_keys)[0])
    if flag is None:
        return
    ver = 0
    if flag:
        ver = sp.get("snes_ksp_ew_version", 2)
        if "snes_ksp_ew_version" in sp:
            used.add("snes_ksp_ew_version")
        if isinstance(ver, bool) or ver not in (1, 2, 3):
            raise ValueError("snes_ksp_ew_version = %r: 1 or 2 (3 is not implemented)" % (ver,))
        if ver == 3:
            raise NotImplementedError("snes_ksp_ew_version 3 is not implemented: it needs the line search's predicted and actual "
                                      "reduction; versions 1 and 2 are")
    _set_checked(o, "ksp_ew", ver, given, "Eisenstat-Walker", "ksp_ew = %r, but snes_ksp_ew = %r%s says %s"
                 % (o["ksp_ew"], sp["snes_ksp_ew"], " with snes_ksp_ew_version %r" % sp["snes_ksp_ew_version"]
                    if "snes_ksp_ew_version" in sp else "", "version %d" % ver if ver else "off"), norm=ew_version)
    for k_src, k_dst in _EW_KEYS:
        if k_src in sp:
            _set_checked(o, k_dst, sp[k_src], given, "Eisenstat-Walker", "%s = %r, %s = %r" % (k_dst, o[k_dst], k_src, sp[k_src]))
            used.add(k_src)


def _reject_schur_krylov(sp, prefix):
    v = sp.get(prefix + "ksp_type", "preonly")
    if v != "preonly":
        raise NotImplementedError("%sksp_type = %r: %s" % (prefix, v, _SCHUR_WHY))


def _reject_unused(sp, used):
    for k in sp:
        if k in used or k in _IGNORED:
            continue
        raise KeyError("solver parameter %r is not consumed by the hot path (it would be silently ignored)" % k)


def _flatten(d, prefix=""):
    """PETSc semantics: a nested dict is a prefix (``"sub_0_cpr_stage1": v_cycle``)."""
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_flatten(v, prefix + k + "_"))
        else:
            out[prefix + k] = v
    return out


def engine_options(solver_parameters, model_name, decoup="No", vector=False):
    from .engine import BUILD_KEYS, DEFAULT_OPTS
    sp = _flatten(dict(solver_parameters))
    o = dict(DEFAULT_OPTS)
    o["decoup"] = decoup
    o["schur_a11"] = False
    o["schur_selfp"] = False
    o["fs_additive"] = False
    used = set()
    for k in BUILD_KEYS:
        if k in sp:
            o[k] = sp.pop(k)
    # ---- Newton / Krylov (singlephase.py:289-301, twophase.py:416-433) --------------------------------------
    _take(sp, used, "snes_type", ("newtonls",))
    # Firedrake's default line search is `basic`; the reference never sets another one on its Newton-Krylov path
    # (l2 only inside the FAS presets, twophase.py:437): anything but basic would silently change the algorithm
    # the engine's own backtracking search is `bt` (PETSc's newtonls default); l2 / cp are not implemented
    ls = _take(sp, used, "snes_linesearch_type", ("basic", "bt"))
    ls_keys = (("snes_linesearch_order", "ls_order"), ("snes_linesearch_alpha", "ls_alpha"), ("snes_linesearch_max_it", "ls_max_it"),
               ("snes_linesearch_maxstep", "ls_maxstep"), ("snes_linesearch_minlambda", "ls_minlambda"))
    if ls is not None:
        _set_checked(o, "linesearch", ls, solver_parameters, "the line search",
                     "linesearch = %r, snes_linesearch_type = %r" % (o["linesearch"], ls))
    for k_src, k_dst in ls_keys:
        if k_src in sp:
            if o["linesearch"] != "bt":
                raise NotImplementedError("%s without snes_linesearch_type bt: the key belongs to the backtracking search "
                                          "(it would be silently ignored)" % k_src)
            o[k_dst] = sp[k_src]
            used.add(k_src)
    _take_ew(sp, used, o, solver_parameters)
    _take(sp, used, "mat_type", ("aij",))
    ksp = _take(sp, used, "ksp_type", ("fgmres", "gmres", "fbcgs", "bcgs"), "gmres")
    side = _take(sp, used, "ksp_pc_side", ("right",))
    if ksp == "gmres" and side is None:
        raise NotImplementedError("ksp_type gmres without ksp_pc_side: PETSc would precondition from the LEFT; only "
                                  "right-preconditioned (F)GMRES is implemented (the reference sets ksp_pc_side right, "
                                  "singlephase.py:296)")
    if ksp == "bcgs" and side is None:
        raise NotImplementedError("ksp_type bcgs without ksp_pc_side: PETSc would precondition from the LEFT; only "
                                  "right-preconditioned BiCGStab is implemented (ksp_type fbcgs, or bcgs with ksp_pc_side right)")
    # outer Krylov method of the engine: restarted FGMRES, or BiCGStab (under which ksp_gmres_restart is consumed below and
    # has no effect: the newton_krylov dicts carry it)
    o["ksp"] = "bcgs" if ksp in ("fbcgs", "bcgs") else "fgmres"
    # Gram-Schmidt refinement of the outer GMRES (PETSc: KSPGMRESSetCGSRefinementType)
    ref = _take(sp, used, "ksp_gmres_cgs_refinement_type", tuple(_CGS_REFINE))
    if ref is not None:
        _set_checked(o, "ksp_reorth", _CGS_REFINE[ref], solver_parameters, "the Gram-Schmidt refinement",
                     "ksp_reorth = %r, ksp_gmres_cgs_refinement_type = %r" % (o["ksp_reorth"], ref))
    for k_src, k_dst in (("ksp_rtol", "ksp_rtol"), ("ksp_atol", "ksp_atol"), ("ksp_max_it", "ksp_max_it"),
                         ("ksp_gmres_restart", "ksp_restart"), ("snes_max_it", "snes_max_it"),
                         ("snes_rtol", "snes_rtol"), ("snes_atol", "snes_atol"), ("snes_stol", "snes_stol")):
        if k_src in sp:
            o[k_dst] = sp[k_src]
            used.add(k_src)
    pc_type = _take(sp, used, "pc_type", ("fieldsplit", "composite", "bjacobi"))
    if pc_type == "bjacobi":
        # pc_bilu (twophase.py:758-762, singlephase.py:402-406): bjacobi + ILU(levels) is the whole preconditioner
        _take(sp, used, "sub_pc_type", ("ilu",))
        if "sub_pc_type" not in used:
            raise NotImplementedError("pc_type bjacobi: sub_pc_type ilu only (pc_bilu)")
        levels = int(_take(sp, used, "sub_pc_factor_levels", None, 0))
        if levels not in (0, 1):
            raise NotImplementedError("bjacobi sub-solver is block-ILU(0) or block-ILU(1) (sub_pc_factor_levels %d)" % levels)
        o["ilu_levels"] = levels
        nb = _take(sp, used, "pc_bjacobi_blocks")
        if nb is not None:
            o["bjacobi_blocks"] = int(nb)
        _take(sp, used, "mat_type", ("aij",))
        if o["decoup"] != "No":
            raise NotImplementedError("pc_bilu has no decoupling stage")
        o["pc"] = "bilu"
        _reject_unused(sp, used)
        _check_inner(o)
        return o
    if pc_type is None:
        raise NotImplementedError("pc_type missing: only the composite CPR/CPTR preconditioners and pc_fieldsplit_cd/_a11 "
                                  "are on the hot path")
    if pc_type == "fieldsplit":
        # pc_fieldsplit_cd (singlephase.py:309-319): Schur FULL (or lower / upper / diag) on (p,T), V-cycle on A_pp, ConvDiffSchurPC on S;
        # pc_fieldsplit_a11 (:331-338): A_TT stands in for the Schur complement;
        # pc_fieldsplit_selfp (:322-330): Sp = A_TT - A_Tp diag(A_pp)^-1 A_pT
        if _take(sp, used, "pc_fieldsplit_type", ("schur", "additive")) == "additive":
            # pc_fieldsplit_diag (singlephase.py:371-375): block-diagonal, one V-cycle on A_pp and one on A_TT
            _take_inner(sp, "fieldsplit_0_", used, o)
            _take_vcycle(sp, "fieldsplit_1_", used, schur="additive")
            if model_name == "Two-phase" or o["decoup"] != "No":
                raise NotImplementedError("pc_fieldsplit_diag is a single-phase preconditioner without decoupling")
            o["pc"], o["schur_a11"], o["fs_additive"] = "fieldsplit_cd", True, True
            _reject_unused(sp, used)
            _check_inner(o)
            return o
        fact = _take_schur_fact(sp, used, "", o, solver_parameters)
        pre = _take(sp, used, "pc_fieldsplit_schur_precondition", ("a11", "selfp"))
        if "pc_fieldsplit_type" not in used or not fact:
            raise NotImplementedError("fieldsplit preconditioners on the hot path: schur with pc_fieldsplit_schur_fact_type FULL, "
                                      "lower, upper or diag and ConvDiffSchurPC (pc_fieldsplit_cd), a11 (pc_fieldsplit_a11) or "
                                      "selfp (pc_fieldsplit_selfp)")
        _take_inner(sp, "fieldsplit_0_", used, o)
        if pre in ("a11", "selfp"):
            _take_vcycle(sp, "fieldsplit_1_", used, schur=True)
        else:
            _reject_schur_krylov(sp, "fieldsplit_1_")
            _take(sp, used, "fieldsplit_1_ksp_type", ("preonly",))
            _take(sp, used, "fieldsplit_1_pc_type", ("python",))
            if not str(_take(sp, used, "fieldsplit_1_pc_python_type", None, "")).endswith("ConvDiffSchurPC"):
                raise NotImplementedError("fieldsplit_1 must be ConvDiffSchurPC (pc_fieldsplit_cd) or a V-cycle "
                                          "(pc_fieldsplit_a11, pc_fieldsplit_selfp)")
            _take_vcycle(sp, "fieldsplit_1_schur_", used, schur=True)
        o["schur_a11"] = pre == "a11"
        o["schur_selfp"] = pre == "selfp"                # (singlephase.py:322-330)
        if model_name == "Two-phase":
            raise NotImplementedError("pc_fieldsplit_cd is the single-phase block preconditioner")
        if o["decoup"] != "No":
            raise NotImplementedError("pc_fieldsplit_cd has no decoupling stage")
        o["pc"] = "fieldsplit_cd"
        _reject_unused(sp, used)
        _check_inner(o)
        return o
    # ---- composite multiplicative (stage 1, bjacobi/ILU(0)) -----------------------------------------------------
    _take(sp, used, "pc_composite_type", ("multiplicative",))
    if not isinstance(o["pc_ctr"], bool):
        raise ValueError("pc_ctr = %r: False or True" % (o["pc_ctr"],))
    sp, pcs, order, given, has_t = _composite_stages(sp, used, ctr=o["pc_ctr"], two_phase=model_name == "Two-phase")
    # (a trailing temperature-only entry needs pc_ctr: True beside it and was stripped; the key alone appends the stage to any dict)
    if has_t and "pc_order" in solver_parameters and order != "SI" and o["pc_order"] != order:
        raise NotImplementedError("pc_composite_pcs = %r ends its sequence %r with the temperature-only stage, but pc_order = %r "
                                  "asks for another sequence, which that stage would not end" % (given, order + "T", o["pc_order"]))
    # the build key pc_order re-orders a dict written in the presets' order "S,I"; a dict that spells another order must agree
    if order != "SI" or "pc_order" not in solver_parameters:
        _set_checked(o, "pc_order", order, solver_parameters, "the order of the composite's stages",
                     "pc_order = %r, pc_composite_pcs = %r" % (o["pc_order"], given))
    if order != "SI":
        # the stages were renamed to the places they have in "S,I" (sub_0_ = S, sub_1_ = I): say so in whatever is raised below
        try:
            return _engine_options_composite(sp, used, o, pcs, model_name, vector, s_moved=not order.startswith("S"),
                                             given=solver_parameters)
        except (KeyError, NotImplementedError, ValueError) as e:
            msg = e.args[0] if e.args else ""
            raise type(e)("%s [pc_composite_pcs = %r: keys are named here by stage, sub_0_ = the %s entry's sub_%d_, sub_1_ = "
                          "the bjacobi entry's sub_%d_]" % (msg, given, pcs.split(",")[0], order.index("S"), order.index("I"))) from e
    return _engine_options_composite(sp, used, o, pcs, model_name, vector, given=solver_parameters)


def _composite_stages(sp, used, ctr=False, two_phase=False):
    """pc_composite_pcs by PETSc's grammar: a comma-separated list of PC type names (blanks ignored, one trailing comma allowed)
    whose k-th entry is configured under the prefix sub_k_.  The hot path has two stages, S = the python / fieldsplit entry
    (CPR, CPTR, the system V-cycle) and I = bjacobi, in the orders S,I | I,S | I,S,I | S,I,S.  Returns the options with every
    stage's keys moved to the prefix it has in "S,I" (S: sub_0_, I: sub_1_), the value in that canonical spelling, the order
    and the value as given.  An entry that appears twice must be configured identically both times: one set-up serves both."""
    if "pc_composite_pcs" not in sp:
        raise NotImplementedError("pc_composite_pcs missing")
    given = sp["pc_composite_pcs"]
    used.add("pc_composite_pcs")
    text = "".join(str(given).split())
    names = (text[:-1] if text.endswith(",") else text).split(",")
    kinds = "".join(_STAGE_OF.get(n, "?") for n in names)
    s_names = sorted({n for n in names if _STAGE_OF.get(n) == "S"})
    prefixes = ["sub_%d_" % k for k in range(len(names))]
    entry = [{k[len(pre):]: v for k, v in sp.items() if k.startswith(pre)} for pre in prefixes]
    # (the reference's cprctr dicts: a third entry that is one V-cycle on field 1 alone, behind a stage on field 0)
    t_at = [k for k, n in enumerate(names)
            if n == "fieldsplit" and "".join(str(entry[k].get("pc_fieldsplit_0_fields", "")).split()) == "1"]
    if t_at and not ctr:
        k = t_at[0]
        raise NotImplementedError("pc_composite_pcs = %r: entry %d (sub_%d_) is a temperature-only stage, a V-cycle on field 1 "
                                  "alone (sub_%d_pc_fieldsplit_0_fields = \"1\"): a third kind of stage is not implemented "
                                  "unless the build key pc_ctr: True stands in the same dict, which runs it as the last stage"
                                  % (given, k, k, k))
    if t_at:
        # pc_ctr: ONE trailing T entry is validated key by key and stripped; the remaining entries map as without it
        if len(t_at) > 1:
            raise NotImplementedError("pc_composite_pcs = %r: entries %s are all temperature-only stages; pc_ctr runs one, as the "
                                      "last stage" % (given, ", ".join("%d" % k for k in t_at)))
        k = t_at[0]
        if k != len(names) - 1:
            raise NotImplementedError("pc_composite_pcs = %r: entry %d (sub_%d_) is a temperature-only stage in the middle of the "
                                      "sequence; pc_ctr runs it as the last stage only" % (given, k, k))
        _take_ctr_entry(sp, prefixes[k], used, two_phase)
        sp = {q: v for q, v in sp.items() if not q.startswith(prefixes[k])}
        names, prefixes, entry = names[:k], prefixes[:k], entry[:k]
        kinds = kinds[:k]
        s_names = sorted({n for n in names if _STAGE_OF.get(n) == "S"})
    if "?" in kinds or kinds not in _ORDERS or len(s_names) != 1:
        raise NotImplementedError("pc_composite_pcs = %r is not implemented on the hot path (supported, X = python or fieldsplit: "
                                  "'X,bjacobi', 'bjacobi,X', 'bjacobi,X,bjacobi', 'X,bjacobi,X')" % (given,))
    first = {"S": kinds.index("S"), "I": kinds.index("I")}
    for k, kind in enumerate(kinds):
        j = first[kind]
        if k == j:
            continue
        a, b = dict(entry[j]), dict(entry[k])
        if kind == "I":         # PETSc's defaults where a key is unset: the same fill level and block count is what matters
            for e in (a, b):
                e.setdefault("sub_pc_type", "ilu")
                e["sub_pc_factor_levels"] = int(e.get("sub_pc_factor_levels", 0))
        diff = sorted(q for q in set(a) | set(b) if a.get(q, _MISSING) != b.get(q, _MISSING))
        if diff:
            raise NotImplementedError("pc_composite_pcs = %r: the two %s entries differ in %s; one set-up serves both, so they "
                                      "must be configured identically" % (given, names[k],
                                      ", ".join("sub_%d_%s / sub_%d_%s" % (j, q, k, q) for q in diff)))
    out = {k: v for k, v in sp.items() if not k.startswith("sub_")}
    for k, v in sp.items():
        if not k.startswith("sub_"):
            continue
        for i, pre in enumerate(prefixes):
            if k.startswith(pre):
                if i == first[kinds[i]]:                 # (a repeated entry equals its first occurrence: dropped)
                    out[("sub_0_" if kinds[i] == "S" else "sub_1_") + k[len(pre):]] = v
                break
        else:
            out[k] = v                                   # no entry has this prefix: left for _reject_unused
    return out, s_names[0] + ",bjacobi", kinds, given, bool(t_at)


def _take_ctr_entry(sp, prefix, used, two_phase):
    """The composite's trailing temperature-only entry under ``prefix`` (the reference's cprctr dicts; engine key pc_ctr): an
    additive fieldsplit whose first split is field 1 with exactly one V-cycle and whose second split, the remaining fields,
    returns zero (gmres, max_it 0, pc none).  Every key is consumed or raises."""
    if not _take_zero_split(sp, used, prefix):
        raise NotImplementedError("%s: the temperature-only stage is pc_fieldsplit_type additive with fieldsplit_1 = gmres, "
                                  "ksp_max_it 0, pc_type none (a second split that returns zero)" % prefix)
    used.add(prefix + "pc_fieldsplit_0_fields")
    rest = _take(sp, used, prefix + "pc_fieldsplit_1_fields")
    want = "0,2" if two_phase else "0"
    if rest is not None and "".join(str(rest).split()) != want:
        raise NotImplementedError("%spc_fieldsplit_1_fields = %r: the remaining fields of the %s model are %r"
                                  % (prefix, rest, "two-phase" if two_phase else "single-phase", want))
    _take_vcycle(sp, prefix + "fieldsplit_0_", used, schur="ctr")
    for k in sp:
        if k.startswith(prefix) and k not in used:
            raise KeyError("solver parameter %r is not consumed by the temperature-only stage (it would be silently ignored)" % k)


def _engine_options_composite(sp, used, o, pcs, model_name, vector, s_moved=False, given=()):
    """The composite's two stages, S under sub_0_ and I under sub_1_ (engine_options); given: the dict as the caller wrote it."""
    if s_moved and "sub_0_cpr_decoup" in sp:
        # the model class reads sub_0_cpr_decoup, the S entry's key only when S comes first: elsewhere the entry's own key decides
        if o["decoup"] not in ("No", sp["sub_0_cpr_decoup"]):
            raise ValueError("the decoupling is configured twice and differently: %r and the stage's cpr_decoup = %r"
                             % (o["decoup"], sp["sub_0_cpr_decoup"]))
        o["decoup"] = sp["sub_0_cpr_decoup"]
    # stage 2: bjacobi + ILU(0) (singlephase.py:348-349); block count: see engine.tiles_for_blocks
    _take(sp, used, "sub_1_sub_pc_type", ("ilu",))
    levels = int(_take(sp, used, "sub_1_sub_pc_factor_levels", None, 0))
    if levels not in (0, 1):
        raise NotImplementedError("stage 2 is block-ILU(0) or block-ILU(1) (sub_1_sub_pc_factor_levels %d)" % levels)
    o["ilu_levels"] = levels
    nb = _take(sp, used, "sub_1_pc_bjacobi_blocks")
    if nb is not None:
        o["bjacobi_blocks"] = int(nb)
    _take(sp, used, "sub_0_cpr_decoup", ("No", "QI", "TI", "QI_temp", "TI_temp"))    # read by the model class (:441-444)
    if pcs == "fieldsplit,bjacobi":
        # the reference's pure-PETSc emulations of its python stage-1 classes (singlephase.py:355-368,
        # twophase.py:619-634,670-699): additive fieldsplit whose second split is "gmres, max_it 0, pc none" -- i.e.
        # returns zero, exactly the y_nonp = 0 of CPRStage1PC/CPTRStage1PC.apply -- with decoupling "No".
        # pc_cpr_gmres == pc_cpr and pc_cptr_gmres == pc_cptr (the two-phase default, twophase.py:930) as algebra.
        if not _take_zero_split(sp, used, "sub_0_"):
            raise NotImplementedError("fieldsplit,bjacobi composite: only the *_gmres emulations of pc_cpr / pc_cptr")
        if o["decoup"] != "No":
            raise NotImplementedError("the fieldsplit emulations have no decoupling stage")
        f0 = _take(sp, used, "sub_0_pc_fieldsplit_0_fields", None, "0")
        f1 = _take(sp, used, "sub_0_pc_fieldsplit_1_fields")
        first = _take(sp, used, "sub_0_fieldsplit_0_pc_type", ("hypre", "fieldsplit"))
        if first == "hypre":
            if f0 != "0":
                raise NotImplementedError("one AMG V-cycle on an explicit multi-field split is not on the hot path")
            _take_inner(sp, "sub_0_fieldsplit_0_", used, o)
            if model_name == "Two-phase" and vector and "sub_0_pc_fieldsplit_0_fields" not in used:
                # pc_cptramg_gmres (twophase.py:698-713): no explicit fields, so with vector=True (forced at :953-955) the
                # splits are the function space's own sub-spaces: (p,T) interleaved | S_o -- ONE V-cycle on the (p,T) system
                o["pc"] = "cptramg"
            else:
                o["pc"] = "cpr"
        elif first == "fieldsplit":
            _take(sp, used, "sub_0_fieldsplit_0_pc_fieldsplit_type", ("schur",))
            fact = _take_schur_fact(sp, used, "sub_0_fieldsplit_0_", o, given)
            _reject_schur_krylov(sp, "sub_0_fieldsplit_0_fieldsplit_1_")
            _take(sp, used, "sub_0_fieldsplit_0_fieldsplit_1_ksp_type", ("preonly",))
            _take(sp, used, "sub_0_fieldsplit_0_fieldsplit_1_pc_type", ("python",))
            py = str(_take(sp, used, "sub_0_fieldsplit_0_fieldsplit_1_pc_python_type", None, ""))
            if not fact:
                raise NotImplementedError("sub_0_fieldsplit_0_pc_fieldsplit_schur_fact_type = %r: the Schur split of the "
                                          "fieldsplit,bjacobi composite is FULL, lower, upper or diag"
                                          % (sp.get("sub_0_fieldsplit_0_pc_fieldsplit_schur_fact_type"),))
            if "sub_0_fieldsplit_0_pc_fieldsplit_type" not in used or not py.endswith("ConvDiffSchurTwoPhasesPC"):
                raise NotImplementedError("unsupported first split of the fieldsplit,bjacobi composite")
            if f0 not in ("0,1", "0, 1") or f1 not in (None, "2"):
                raise NotImplementedError("pc_cptr_gmres splits fields (0,1 | 2)")
            _take_inner(sp, "sub_0_fieldsplit_0_fieldsplit_0_", used, o)
            _take_vcycle(sp, "sub_0_fieldsplit_0_fieldsplit_1_schur_", used, schur=True)
            if model_name != "Two-phase":
                raise NotImplementedError("pc_cptr_gmres needs the two-phase model")
            o["pc"] = "cptr"
        else:
            raise NotImplementedError("unsupported first split of the fieldsplit,bjacobi composite "
                                      "(mg/LU/system-AMG variants are not on the hot path)")
        _reject_unused(sp, used)
        _check_inner(o)
        return o
    pytype = str(_take(sp, used, "sub_0_pc_python_type", None, ""))
    if pytype.endswith("CPRStage1PC"):
        o["pc"] = "cpr"
        _take_inner(sp, "sub_0_cpr_stage1_", used, o)
    elif pytype.endswith("CPTRStage1PC"):
        if model_name != "Two-phase":
            raise NotImplementedError("CPTRStage1PC needs the two-phase model")
        kind = _take(sp, used, "sub_0_cpr_stage1_pc_type", ("fieldsplit", "hypre", "ksp"))
        if kind == "ksp":
            # PCKSP around the stage-1 solver: only around the system V-cycle (an iteration around the whole Schur fieldsplit
            # would nest the pressure and temperature solves in every inner mat-vec)
            if sp.get("sub_0_cpr_stage1_ksp_pc_type") != "hypre":
                raise NotImplementedError("sub_0_cpr_stage1_pc_type ksp: only around the (p,T) system V-cycle (sub_0_cpr_stage1_"
                                          "ksp_pc_type hypre, pc_cptramg*); for pc_cptr put the inner solver on "
                                          "sub_0_cpr_stage1_fieldsplit_0_")
            kind = "hypre"
        if kind is None:
            raise NotImplementedError("CPTRStage1PC needs sub_0_cpr_stage1_pc_type fieldsplit (pc_cptr) or hypre "
                                      "(pc_cptramg*); the LU variants (pc_cptrlu*) are not on the hot path")
        if kind == "hypre":
            # pc_cptramg[_QI|_TI] (twophase.py:552-566): ONE BoomerAMG V-cycle on the interleaved (p,T) system
            o["pc"] = "cptramg"
            _take_inner(sp, "sub_0_cpr_stage1_", used, o, ksp_default="preonly")
            if o["decoup"] not in ("No", "QI", "TI"):
                raise NotImplementedError("pc_cptramg: decoupling No, QI or TI (twophase.py:552-566)")
        else:
            o["pc"] = "cptr"
            _take(sp, used, "sub_0_cpr_stage1_pc_fieldsplit_type", ("schur",))
            fact = _take_schur_fact(sp, used, "sub_0_cpr_stage1_", o, given)
            if "sub_0_cpr_stage1_pc_fieldsplit_type" not in used or not fact:
                raise NotImplementedError("CPTR stage 1: fieldsplit schur with pc_fieldsplit_schur_fact_type FULL, lower, upper or "
                                          "diag (twophase.py:536-538)")
            pre = _take(sp, used, "sub_0_cpr_stage1_pc_fieldsplit_schur_precondition", ("a11",))
            o["schur_a11"] = pre == "a11"                   # pc_cptr_a11 (twophase.py:598-616)
            _take_inner(sp, "sub_0_cpr_stage1_fieldsplit_0_", used, o)
            if pre == "a11":
                _take_vcycle(sp, "sub_0_cpr_stage1_fieldsplit_1_", used, schur=True)
            else:
                _reject_schur_krylov(sp, "sub_0_cpr_stage1_fieldsplit_1_")
                _take(sp, used, "sub_0_cpr_stage1_fieldsplit_1_ksp_type", ("preonly",))
                _take(sp, used, "sub_0_cpr_stage1_fieldsplit_1_pc_type", ("python",))
                py = str(_take(sp, used, "sub_0_cpr_stage1_fieldsplit_1_pc_python_type", None, ""))
                if not py.endswith("ConvDiffSchurTwoPhasesPC"):
                    raise NotImplementedError("CPTR stage 1: the Schur split must be ConvDiffSchurTwoPhasesPC or a11")
                _take_vcycle(sp, "sub_0_cpr_stage1_fieldsplit_1_schur_", used, schur=True)
    else:
        raise NotImplementedError("sub_0_pc_python_type %r" % pytype)
    if o["decoup"] not in ("No", "QI", "TI", "QI_temp", "TI_temp"):
        raise NotImplementedError("unknown decoupling %r" % o["decoup"])
    if o["decoup"].endswith("_temp") and (o["pc"] != "cpr" or model_name != "Two-phase"):
        raise NotImplementedError("QI_temp/TI_temp decouple temperature AND saturation from the pressure: "
                                  "two-phase pc_cpr only (preconditioners.py:367-368)")
    _reject_unused(sp, used)
    _check_inner(o)
    return o
