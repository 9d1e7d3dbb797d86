"""Regenerates options_golden.json: what the option plumbing does, recorded from the code as it stood at the commit named in
the file (tests/test_options_golden.py replays it against the code under test).

Every dict is stored as a change of another one (tests/optpack.py: delta, expand): the engine options as changes of `defaults`, a
solver_parameters dict as a change of the earlier case `like`; the packed bytes whole for the first case and as the fields that
differ from it for the others.

  pack   engine option dicts and the bytes HipEngine._make_options packs them into (ctypes zero-fills padding): the defaults, every
         key that reaches tp_options with a non-default value (every member of every enumeration), the derived encodings, the dict
         with each optional key missing, and every key non-default at once
  map    PETSc-style solver_parameters -> engine options (solver_options.engine_options): every string preset of SinglePhase and
         TwoPhase, and hand-written dicts that say an option twice (build key and PETSc spelling), once agreeing and once not;
         for a refused dict the exception's [type name, message] stands in place of the options

The fixture pins behaviour ACROSS changes of the plumbing, so it is not regenerated with them: regenerating is legitimate only
when tp_options itself changes (a field added, removed or re-encoded), and then from the commit before the plumbing is touched.
usage: python tests/golden/make_options_golden.py
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

from optpack import delta, differing_fields, expand, field_bytes, patched   # noqa: E402
from oracle.engine import OracleEngine                                      # noqa: E402
from thermalporous_amd.engine import DEFAULT_OPTS, HipEngine, tp_options    # noqa: E402
from thermalporous_amd.homogeneousgeo import HomogeneousGeo                 # noqa: E402
from thermalporous_amd.physicalparameters import PhysicalParameters         # noqa: E402
from thermalporous_amd.singlephase import SinglePhase                       # noqa: E402
from thermalporous_amd.solver_options import engine_options                 # noqa: E402
from thermalporous_amd.twophase import TwoPhase                             # noqa: E402
from thermalporous_amd.wellcase import WellCase                             # noqa: E402

BIG = 1 << 30
D = dict(DEFAULT_OPTS, ilu_tile=(BIG, 8, 8))
DEFAULTS = json.loads(json.dumps(DEFAULT_OPTS))

# key -> valid non-default values (the default itself where another spelling of it packs the same bytes: 0 / False)
VALUES = dict(
    pc=["cpr", "cptr", "fieldsplit_cd", "cptramg", "bilu"], decoup=["No", "QI", "TI", "QI_temp", "TI_temp"],
    pc_order=["SI", "IS", "ISI", "SIS"], pc_ctr=[True], ksp_rtol=[1e-9], ksp_atol=[1e-30], ksp_max_it=[150], ksp_restart=[30],
    ksp=["fgmres", "bcgs"], ksp_basis_single=[True], ksp_single_floor=[1e-5], ksp_reorth=["never", "ifneeded", "always"],
    ksp_reorth_eta=[0.5], snes_rtol=[1e-6], snes_atol=[1e-40], snes_stol=[1e-7], snes_max_it=[9], amg_omega=[0.8],
    amg_min_cells=[32], amg_nu=[3], amg_full_levels=[2], amg_coarse_pre=[1], amg_coarse_post=[2], amg_mid_skip=[True, 1, 0, False],
    amg_tail_post=[3], amg_single=[False, 0, 1, True], amg_dom_tau=[0.1], amg_line_levels=[2], amg_gs_levels=[2], amg_gs_sweeps=[3],
    amg_gather_cells=[1000], schur_a11=[True], fs_additive=[True], schur_selfp=[True],
    schur_fact=["full", "lower", "upper", "diag"], schur_scale=[0.5],
    ilu_tile=[(BIG, 8, 8), (12, 6, 9), (BIG, 100, 70)],                     # t0 = 1 << 30 -> 0, a finite t0, t1 / t2 clipped to 64
    ilu_levels=[1], ilu_block=[None, (4, 5, 6), (1 << 31, 30, 55)],         # 1 << 31 clipped to 1 << 30
    ilu_single=[True], ilu_whole=[True], s1_ksp=["preonly", "richardson", "fgmres"], s1_max_it=[5], s1_rtol=[1e-3], s1_atol=[1e-20],
    linesearch=["basic", "bt"], ls_order=[2], ls_alpha=[1e-3], ls_max_it=[10], ls_maxstep=[1e3], ls_minlambda=[1e-6],
    ls_max_change=[None, (1e5, 10.0, 0.1)], ksp_ew=[False, 0, 1, 2, True], ew_rtol0=[0.1], ew_rtolmax=[0.5], ew_gamma=[0.9],
    ew_alpha=[2.0], ew_alpha2=[1.5], ew_threshold=[0.2],
)
# the keys HipEngine._make_options read through o.get(...) at the recorded commit (read off the function): a dict without one of
# them packs as the fallback written there
OPTIONAL = ("schur_selfp", "amg_dom_tau", "ilu_levels", "fs_additive", "ilu_whole", "amg_gs_levels", "amg_gs_sweeps", "ilu_block",
            "ilu_single", "amg_line_levels", "ksp_basis_single", "ksp_single_floor", "ksp", "s1_ksp", "s1_max_it", "s1_rtol",
            "s1_atol", "ew_rtol0", "ew_rtolmax", "ew_gamma", "ew_alpha", "ew_alpha2", "ew_threshold", "ksp_ew", "pc_order", "pc_ctr",
            "schur_fact", "schur_scale", "ksp_reorth", "ksp_reorth_eta", "linesearch", "ls_order", "ls_max_it", "ls_alpha",
            "ls_maxstep", "ls_minlambda", "ls_max_change")


def pack_cases():
    corpus = [D] + [dict(D, **{k: v}) for k, vs in VALUES.items() for v in vs]
    corpus += [{q: v for q, v in D.items() if q != k} for k in OPTIONAL]
    corpus.append(dict(D, **{k: vs[-1] for k, vs in VALUES.items()}))       # every key non-default at once
    out, first = [], None
    for o in corpus:
        o = json.loads(json.dumps(o))                                       # as the test will read it: tuples are lists
        t = HipEngine._make_options(o)
        case = delta(o, DEFAULTS)
        assert expand(DEFAULTS, case) == o and json.dumps(expand(DEFAULTS, case), sort_keys=True) == json.dumps(o, sort_keys=True)
        if first is None:
            first = t
            case["hex"] = bytes(t).hex()
        else:
            case["fields"] = {n: field_bytes(t, n).hex() for n in sorted(differing_fields(t, first))}
            assert patched(bytes(first), tp_options, case["fields"]) == bytes(t)
        out.append(case)
    return out


# ---- PETSc dicts ----------------------------------------------------------------------------------------------------------------
PRESETS = {False: ("pc_cpr", "pc_cpr_QI", "pc_cpr_TI", "pc_cpr_gmres", "pc_bilu", "pc_fieldsplit_cd", "pc_fieldsplit_a11",
                   "pc_fieldsplit_selfp", "pc_fieldsplit_diag"),
           True: ("pc_cptr", "pc_cptr_a11", "pc_cpr", "pc_cpr_QI", "pc_cpr_TI", "pc_cpr_QI_temp", "pc_cpr_TI_temp", "pc_cpr_gmres",
                  "pc_cptr_gmres", "pc_cprilu1_gmres", "pc_bilu", "pc_cptramg_gmres", "pc_cptramg", "pc_cptramg_QI", "pc_cptramg_TI")}


def model(name, two_phase):
    p = PhysicalParameters()
    if two_phase:
        p.S_o = 0.9
    g = HomogeneousGeo(8, 8, p, 20., 20.)
    c = WellCase(p, g, well_case="test0", constant_rate=True)
    return (TwoPhase if two_phase else SinglePhase)(g, c, p, solver_parameters=name, filename=None, verbosity=False,
                                                    _engine_factory=OracleEngine)


V = {"ksp_type": "preonly", "pc_type": "hypre", "pc_hypre_type": "boomeramg", "pc_hypre_boomeramg_max_iter": 1}
NK = {"snes_type": "newtonls", "ksp_type": "fgmres", "mat_type": "aij"}
COMPOSITE = dict(NK, pc_type="composite", pc_composite_type="multiplicative")
ILU = {"sub_1_sub_pc_type": "ilu", "sub_1_sub_pc_factor_levels": 0}
BILU = dict(NK, pc_type="bjacobi", sub_pc_type="ilu")
CPR = dict(COMPOSITE, pc_composite_pcs="python,bjacobi", sub_0_pc_python_type="thermalporous.preconditioners.CPRStage1PC",
           sub_0_cpr_stage1=dict(V), **ILU)
S1 = "sub_0_cpr_stage1_"
CPTR = dict(COMPOSITE, pc_composite_pcs="python,bjacobi", **ILU, **{
    "sub_0_pc_python_type": "thermalporous.preconditioners.CPTRStage1PC", S1 + "pc_type": "fieldsplit",
    S1 + "pc_fieldsplit_type": "schur", S1 + "pc_fieldsplit_schur_fact_type": "FULL", S1 + "fieldsplit_0": dict(V),
    S1 + "fieldsplit_1_ksp_type": "preonly", S1 + "fieldsplit_1_pc_type": "python",
    S1 + "fieldsplit_1_pc_python_type": "thermalporous.preconditioners.ConvDiffSchurTwoPhasesPC", S1 + "fieldsplit_1_schur": dict(V)})
KF, KS = S1 + "pc_fieldsplit_schur_fact_type", S1 + "pc_fieldsplit_schur_scale"


def split_entry(k, f0, f1):
    """An additive fieldsplit entry: one V-cycle on the fields f0, zero on the fields f1 (gmres, max_it 0, pc none)."""
    p = "sub_%d_" % k
    return {p + "pc_fieldsplit_type": "additive", p + "pc_fieldsplit_0_fields": f0, p + "pc_fieldsplit_1_fields": f1,
            p + "fieldsplit_0": dict(V), p + "fieldsplit_1_ksp_type": "gmres", p + "fieldsplit_1_ksp_max_it": 0,
            p + "fieldsplit_1_pc_type": "none"}


def ilu_entry(k, levels=0):
    return {"sub_%d_sub_pc_type" % k: "ilu", "sub_%d_sub_pc_factor_levels" % k: levels}


IS = dict(COMPOSITE, pc_composite_pcs="bjacobi,python", **ilu_entry(0), sub_1_pc_python_type=CPR["sub_0_pc_python_type"],
          sub_1_cpr_stage1=dict(V))
ISI = dict(COMPOSITE, pc_composite_pcs="bjacobi, fieldsplit ,bjacobi,", **ilu_entry(0, 1), **split_entry(1, "0", "1,2"),
           **ilu_entry(2, 1), sub_0_pc_bjacobi_blocks=4, sub_2_pc_bjacobi_blocks=4)
CTR = dict(COMPOSITE, pc_composite_pcs="fieldsplit,bjacobi,fieldsplit", pc_ctr=True, **split_entry(0, "0", "1,2"), **ilu_entry(1),
           **split_entry(2, "1", "0,2"))
PCKSP = {k: v for k, v in CPR.items() if k != "sub_0_cpr_stage1"}
PCKSP.update({S1 + "pc_type": "ksp", S1 + "ksp_pc_type": "hypre", S1 + "ksp_pc_hypre_type": "boomeramg",
              S1 + "ksp_pc_hypre_boomeramg_max_iter": 1, S1 + "ksp_ksp_type": "fgmres", S1 + "ksp_ksp_max_it": 6,
              S1 + "ksp_ksp_rtol": 1e-3})
GMRES_EMU = dict(COMPOSITE, pc_composite_pcs="fieldsplit,bjacobi", **split_entry(0, "0", "1,2"), **ilu_entry(1))

# (path, solver_parameters, model name): an accepted and a refused dict per path
HAND = [
    ("linesearch", dict(CPR, linesearch="bt", snes_linesearch_type="bt", snes_linesearch_order=2), "Two-phase"),
    ("linesearch", dict(CPR, linesearch="basic", snes_linesearch_type="bt"), "Two-phase"),
    ("ksp_reorth", dict(BILU, ksp_reorth="always", ksp_gmres_cgs_refinement_type="refine_always"), "Two-phase"),
    ("ksp_reorth", dict(BILU, ksp_reorth="always", ksp_gmres_cgs_refinement_type="refine_never"), "Two-phase"),
    ("schur_fact", {**CPTR, "schur_fact": "upper", KF: "Upper"}, "Two-phase"),
    ("schur_fact", {**CPTR, "schur_fact": "upper", KF: "lower"}, "Two-phase"),
    ("schur_scale", {**CPTR, "schur_scale": 2.0, KF: "diag", KS: 2}, "Two-phase"),
    ("schur_scale", {**CPTR, "schur_scale": 0.5, KF: "diag", KS: 2.0}, "Two-phase"),
    ("ksp_ew", dict(CPR, ksp_ew=1, snes_ksp_ew=None, snes_ksp_ew_version=1), "Two-phase"),
    ("ksp_ew", dict(CPR, ksp_ew=1, snes_ksp_ew=None), "Two-phase"),
    ("ew_rtol0", dict(CPR, ksp_ew=2, snes_ksp_ew=None, ew_rtol0=0.1, snes_ksp_ew_rtol0=0.1), "Two-phase"),
    ("ew_rtol0", dict(CPR, ksp_ew=2, snes_ksp_ew=None, ew_rtol0=0.1, snes_ksp_ew_rtol0=0.2), "Two-phase"),
    ("pc_order", dict(IS, pc_order="IS"), "Single phase"),
    ("pc_order", dict(IS, pc_order="SIS"), "Single phase"),
    ("s1", {**CPR, "s1_ksp": "richardson", "s1_max_it": 3, "sub_0_cpr_stage1": dict(V, pc_hypre_boomeramg_max_iter=3)}, "Single phase"),
    ("s1", {**CPR, "s1_ksp": "fgmres", "s1_max_it": 4, "sub_0_cpr_stage1": dict(V, pc_hypre_boomeramg_max_iter=2)}, "Single phase"),
    ("pc_ctr entry", CTR, "Two-phase"),
    ("pc_ctr entry", dict(CTR, sub_2_fieldsplit_1_ksp_max_it=1), "Two-phase"),
    ("ISI composite", ISI, "Two-phase"),
    ("ISI composite", dict(ISI, sub_1_bogus=1), "Two-phase"),
    ("pc_type ksp", PCKSP, "Single phase"),
    ("pc_type ksp", {**PCKSP, S1 + "ksp_ksp_type": "gmres"}, "Single phase"),
    ("bjacobi", dict(BILU, sub_pc_factor_levels=1, pc_bjacobi_blocks=4), "Two-phase"),
    ("bjacobi", dict(BILU, sub_pc_type="lu"), "Two-phase"),
    ("fieldsplit,bjacobi zero split", GMRES_EMU, "Two-phase"),
    ("fieldsplit,bjacobi zero split", dict(GMRES_EMU, sub_0_fieldsplit_1_ksp_max_it=1), "Two-phase"),
]


def outcome(sp, name, decoup, vector):
    try:
        return engine_options(sp, name, decoup, vector)
    except (NotImplementedError, ValueError, KeyError) as e:
        return [type(e).__name__, e.args[0]]


def map_cases():
    out = []
    for two_phase, names in PRESETS.items():
        for preset in names:
            m = model(preset, two_phase)
            vector = bool(getattr(m, "vector", False))
            assert m.engine_opts == engine_options(m.solver_parameters, m.name, m.decoup, vector)
            out.append({"name": "%s %s" % (m.name, preset), "sp": m.solver_parameters, "model": m.name, "decoup": m.decoup,
                        "vector": vector, "out": m.engine_opts})
    for path, sp, name in HAND:
        out.append({"name": path, "sp": sp, "model": name, "decoup": "No", "vector": False, "out": outcome(sp, name, "No", False)})
    kinds = [isinstance(c["out"], list) for c in out[-len(HAND):]]
    assert kinds == [False, True]*(len(HAND)//2), kinds                     # each path: accepted, then refused
    out, full = json.loads(json.dumps(out)), []
    for i, c in enumerate(out):                 # sp as a change of the earlier case that makes it shortest, out of the defaults
        sp, c["like"] = c.pop("sp"), None
        best = delta(sp, {})
        for j in range(i):
            d = delta(sp, full[j])
            if len(json.dumps(d)) < len(json.dumps(best)):
                best, c["like"] = d, j
        full.append(sp)
        c.update(best)
        if isinstance(c["out"], dict):
            d = delta(c["out"], DEFAULTS)
            assert json.dumps(expand(DEFAULTS, d), sort_keys=True) == json.dumps(c["out"], sort_keys=True)
            c["out"] = d
    return out


if __name__ == "__main__":
    root = os.path.join(HERE, "..", "..")
    commit = subprocess.check_output(["git", "-C", root, "rev-parse", "HEAD"], text=True).strip()
    blob = {"commit": commit, "defaults": DEFAULTS, "pack": pack_cases(), "map": map_cases()}
    path = os.path.join(HERE, "options_golden.json")
    with open(path, "w") as f:
        f.write('{"commit": %s,\n"defaults": %s,\n"pack": [\n%s\n],\n"map": [\n%s\n]}\n' % (
            json.dumps(commit), json.dumps(DEFAULTS), ",\n".join(json.dumps(c) for c in blob["pack"]),
            ",\n".join(json.dumps(c) for c in blob["map"])))
    assert json.load(open(path)) == blob
    print("wrote options_golden.json at %s: %d pack cases, %d map cases, %d bytes"
          % (commit[:7], len(blob["pack"]), len(blob["map"]), os.path.getsize(path)))
