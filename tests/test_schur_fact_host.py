"""Factorisation types of the Schur split on (p,T) (schur_fact / schur_scale): what can be checked without a GPU
-- the three PETSc keys and the scale through the option parser, every preset with a Schur split under each of the four values,
the refusals, the struct and the export, and the numpy reference tests/schur_fact_ref.py on the six small systems the GPU tests use
(tests/test_gpu_schur_fact.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import schur_fact_ref as SR
from optpack import differing_fields
from oracle.engine import OracleEngine
from thermalporous_amd.engine import (API_SYMBOLS, DEFAULT_OPTS, HipEngine, check_schur_fact_options, tp_options)
from thermalporous_amd.homogeneousgeo import HomogeneousGeo
from thermalporous_amd.physicalparameters import PhysicalParameters
from thermalporous_amd.singlephase import SinglePhase
from thermalporous_amd.solver_options import engine_options
from thermalporous_amd.twophase import TwoPhase
from thermalporous_amd.wellcase import WellCase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "thermalporous_hip.h")
CODES = {"full": 0, "lower": 1, "upper": 2, "diag": 3}
V = {"ksp_type": "preonly", "pc_type": "hypre", "pc_hypre_type": "boomeramg", "pc_hypre_boomeramg_max_iter": 1}
NK = {"snes_type": "newtonls", "ksp_type": "fgmres", "mat_type": "aij"}

# the pc_fieldsplit_cd dict of the reference's single-phase driver script, typed as it stands there (nested v_cycle dicts included)
REF_SCRIPT_CD = {"pc_type": "fieldsplit",
                 "pc_fieldsplit_type": "schur",
                 "pc_fieldsplit_schur_fact_type": "lower",
                 "fieldsplit_0": dict(V),
                 "fieldsplit_1_ksp_type": "preonly",
                 "fieldsplit_1_pc_type": "python",
                 "fieldsplit_1_pc_python_type": "thermalporous.preconditioners.ConvDiffSchurPC",
                 "fieldsplit_1_schur": dict(V)}

# (preset, model, prefix of its fact-type key, expected pc)
PRESETS = [("pc_fieldsplit_cd", "1ph", "", "fieldsplit_cd"), ("pc_fieldsplit_a11", "1ph", "", "fieldsplit_cd"),
           ("pc_fieldsplit_selfp", "1ph", "", "fieldsplit_cd"), ("pc_cptr", "2ph", "sub_0_cpr_stage1_", "cptr"),
           ("pc_cptr_a11", "2ph", "sub_0_cpr_stage1_", "cptr"), ("pc_cptr_gmres", "2ph", "sub_0_fieldsplit_0_", "cptr")]


def preset_dict(preset, model):
    p = PhysicalParameters()
    g = HomogeneousGeo(8, 8, p, 20., 20.)
    c = WellCase(p, g, well_case="test0", constant_rate=True)
    cls = SinglePhase if model == "1ph" else TwoPhase
    m = cls(g, c, p, solver_parameters=preset, filename=None, verbosity=False, _engine_factory=OracleEngine)
    return dict(m.solver_parameters), m.name


# ---- the three keys -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,model,prefix,pc", PRESETS, ids=[p[0] for p in PRESETS])
@pytest.mark.parametrize("fact", SR.FACTS)
def test_every_schur_preset_takes_every_fact_type(preset, model, prefix, pc, fact):
    sp, name = preset_dict(preset, model)
    key = prefix + "pc_fieldsplit_schur_fact_type"
    assert str(sp[key]).upper() == "FULL"
    ref = engine_options(sp, name)
    assert (ref["pc"], ref["schur_fact"], ref["schur_scale"]) == (pc, "full", -1.0)
    # any letter case, as PETSc reads it
    for spelt in (fact, fact.upper(), fact.capitalize()):
        o = engine_options({**sp, key: spelt}, name)
        assert o["schur_fact"] == fact and o["schur_scale"] == -1.0
        # nothing else moves
        assert {k: v for k, v in o.items() if k != "schur_fact"} == {k: v for k, v in ref.items() if k != "schur_fact"}
    # an unknown value, and the key under another prefix
    with pytest.raises(NotImplementedError, match="schur"):
        engine_options({**sp, key: "left"}, name)
    with pytest.raises((KeyError, NotImplementedError)):
        engine_options({**sp, "sub_7_" + key: fact}, name)


def test_the_reference_scripts_dict_loads_as_written():
    o = engine_options({**NK, "ksp_pc_side": "right", **REF_SCRIPT_CD}, "Single phase")
    assert (o["pc"], o["schur_fact"], o["schur_scale"]) == ("fieldsplit_cd", "lower", -1.0)
    assert not o["schur_a11"] and not o["schur_selfp"] and not o["fs_additive"]
    # through the model class, as the script hands it over
    p = PhysicalParameters()
    g = HomogeneousGeo(8, 8, p, 20., 20.)
    m = SinglePhase(g, WellCase(p, g, well_case="test0", constant_rate=True), p, solver_parameters={**NK, "ksp_pc_side": "right", **REF_SCRIPT_CD},
                    filename=None, verbosity=False, _engine_factory=OracleEngine)
    assert (m.engine_opts["pc"], m.engine_opts["schur_fact"]) == ("fieldsplit_cd", "lower")


@pytest.mark.parametrize("preset,model,prefix,pc", PRESETS, ids=[p[0] for p in PRESETS])
def test_the_scale_key_with_and_without_diag(preset, model, prefix, pc):
    sp, name = preset_dict(preset, model)
    kf, ks = prefix + "pc_fieldsplit_schur_fact_type", prefix + "pc_fieldsplit_schur_scale"
    assert engine_options({**sp, kf: "diag", ks: 0.5}, name)["schur_scale"] == 0.5
    assert engine_options({**sp, kf: "DIAG", ks: 1}, name)["schur_scale"] == 1.0
    assert engine_options({**sp, kf: "diag"}, name)["schur_scale"] == -1.0
    for fact in ("FULL", "lower", "upper"):
        with pytest.raises(ValueError, match=r"pc_fieldsplit_schur_scale.*pc_fieldsplit_schur_fact_type"):
            engine_options({**sp, kf: fact, ks: 0.5}, name)
    with pytest.raises(ValueError, match="pc_fieldsplit_schur_scale"):
        engine_options({**sp, kf: "diag", ks: "half"}, name)
    with pytest.raises(ValueError, match="schur_scale"):
        engine_options({**sp, kf: "diag", ks: float("inf")}, name)
    # the scale under another prefix than the fact type's is not consumed
    with pytest.raises(KeyError, match="pc_fieldsplit_schur_scale"):
        engine_options({**sp, kf: "diag", "fieldsplit_9_pc_fieldsplit_schur_scale": 0.5}, name)
    # the build keys
    o = engine_options({**sp, "schur_fact": "diag", "schur_scale": 0.25, kf: "diag"}, name)
    assert (o["schur_fact"], o["schur_scale"]) == ("diag", 0.25)
    with pytest.raises(ValueError, match=r"schur_scale.*schur_fact"):
        engine_options({**sp, "schur_scale": 0.25}, name)


@pytest.mark.parametrize("preset,model,prefix,pc", PRESETS, ids=[p[0] for p in PRESETS])
def test_configured_twice_and_differently(preset, model, prefix, pc):
    sp, name = preset_dict(preset, model)
    kf, ks = prefix + "pc_fieldsplit_schur_fact_type", prefix + "pc_fieldsplit_schur_scale"
    with pytest.raises(ValueError, match=r"twice.*schur_fact.*pc_fieldsplit_schur_fact_type"):
        engine_options({**sp, "schur_fact": "upper", kf: "lower"}, name)
    with pytest.raises(ValueError, match=r"twice.*schur_fact.*pc_fieldsplit_schur_fact_type"):
        engine_options({**sp, "schur_fact": "lower"}, name)               # (the preset says FULL)
    with pytest.raises(ValueError, match=r"twice.*schur_scale.*pc_fieldsplit_schur_scale"):
        engine_options({**sp, "schur_scale": 0.5, kf: "diag", ks: 2.0}, name)
    # twice and the same
    assert engine_options({**sp, "schur_fact": "upper", kf: "Upper"}, name)["schur_fact"] == "upper"
    assert engine_options({**sp, "schur_scale": 2.0, kf: "diag", ks: 2}, name)["schur_scale"] == 2.0


# ---- the option check -------------------------------------------------------------------------------------------------------------
def test_unknown_values_raise():
    for bad in ("FULL", "Lower", "left", "", 1, None, True):
        with pytest.raises(ValueError, match="schur_fact"):
            check_schur_fact_options(dict(DEFAULT_OPTS, pc="cptr", schur_fact=bad))
    for bad in (float("nan"), float("inf"), -float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="schur_scale"):
            check_schur_fact_options(dict(DEFAULT_OPTS, pc="cptr", schur_fact="diag", schur_scale=bad))
    for fact in ("full", "lower", "upper"):
        with pytest.raises(ValueError, match=r"schur_scale.*schur_fact"):
            check_schur_fact_options(dict(DEFAULT_OPTS, pc="cptr", schur_fact=fact, schur_scale=0.5))
    check_schur_fact_options(dict(DEFAULT_OPTS, pc="cptr", schur_fact="diag", schur_scale=0.5))
    check_schur_fact_options(dict(DEFAULT_OPTS, pc="cptr", schur_fact="diag", schur_scale=np.float64(-2)))


@pytest.mark.parametrize("fact", ["lower", "upper", "diag"])
def test_refused_combinations_name_both(fact):
    for pc in ("cpr", "cptramg", "bilu"):
        with pytest.raises(NotImplementedError, match=r"schur_fact.*%s" % pc):
            check_schur_fact_options(dict(DEFAULT_OPTS, pc=pc, schur_fact=fact))
        check_schur_fact_options(dict(DEFAULT_OPTS, pc=pc))                 # the default goes with every preconditioner
    with pytest.raises(NotImplementedError, match=r"schur_fact.*fs_additive"):
        check_schur_fact_options(dict(DEFAULT_OPTS, pc="fieldsplit_cd", schur_a11=True, fs_additive=True, schur_fact=fact))
    # through the PETSc dicts, with the build key
    with pytest.raises(NotImplementedError, match=r"schur_fact.*bilu"):
        engine_options({**NK, "pc_type": "bjacobi", "sub_pc_type": "ilu", "schur_fact": fact}, "Two-phase")
    with pytest.raises(NotImplementedError, match=r"schur_fact.*fs_additive"):
        engine_options({**NK, "pc_type": "fieldsplit", "pc_fieldsplit_type": "additive", "fieldsplit_0": dict(V), "fieldsplit_1": dict(V),
                        "schur_fact": fact}, "Single phase")
    sp, name = preset_dict("pc_cpr", "2ph")
    with pytest.raises(NotImplementedError, match=r"schur_fact.*cpr"):
        engine_options({**sp, "schur_fact": fact}, name)
    # it combines with everything else on the preconditioners that have the split
    for extra in (dict(decoup="QI"), dict(decoup="TI"), dict(schur_a11=True), dict(s1_ksp="fgmres", s1_max_it=3),
                  dict(pc_order="SIS"), dict(pc_order="ISI"), dict(pc_ctr=True), dict(ksp="bcgs"), dict(ksp_basis_single=True),
                  dict(ksp_reorth="always"), dict(ksp_ew=2), dict(linesearch="bt"), dict(amg_single=True), dict(amg_gs_levels=1)):
        check_schur_fact_options(dict(DEFAULT_OPTS, pc="cptr", schur_fact=fact, **extra))
    for extra in (dict(), dict(schur_a11=True), dict(schur_selfp=True)):
        check_schur_fact_options(dict(DEFAULT_OPTS, pc="fieldsplit_cd", schur_fact=fact, **extra))


# ---- struct, header, export --------------------------------------------------------------------------------------------------------
def test_defaults_struct_fields_and_export():
    assert DEFAULT_OPTS["schur_fact"] == "full" and DEFAULT_OPTS["schur_scale"] == -1.0
    types = dict(tp_options._fields_)
    assert types["schur_fact"] is C.c_int32 and types["schur_scale"] is C.c_double
    assert tp_options.schur_scale.offset % C.sizeof(C.c_double) == 0
    names = [f[0] for f in tp_options._fields_]
    i = names.index("schur_fact")
    assert names[i:i + 2] == ["schur_fact", "schur_scale"] and names[-4:] == ["s1_ksp", "s1_max_it", "s1_rtol", "s1_atol"]
    # the header declares the same two fields in the same place, and the export
    text = open(HEADER).read()
    body = text[text.index("typedef struct tp_options {"):text.index("} tp_options;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(?:int32_t|double)\s+(\w+)", body)
    j = fields.index("schur_fact")
    assert fields[j - 1] == names[i - 1] and fields[j:j + 3] == names[i:i + 3]
    assert "int32_t schur_fact;" in text and "double  schur_scale;" in text
    assert "tp_schur_info" in API_SYMBOLS and hasattr(HipEngine, "schur_info")
    assert "int tp_schur_info(tp_ctx *ctx, int *fact, double *scale, long *k0_applies, long *ks_applies);" in text


def test_make_options_encodes_the_four_values():
    base = dict(DEFAULT_OPTS, pc="cptr", ilu_tile=(1 << 30, 8, 8))
    base.pop("schur_fact")
    base.pop("schur_scale")
    a = HipEngine._make_options(base)                       # without the keys
    assert a.schur_fact == 0 and a.schur_scale == -1.0
    for fact, code in CODES.items():
        b = HipEngine._make_options(dict(base, schur_fact=fact))
        assert b.schur_fact == code and b.schur_scale == -1.0
        # every other field is what it was without the key
        assert differing_fields(a, b) <= {"schur_fact"}
    assert HipEngine._make_options(dict(base, schur_fact="diag", schur_scale=0.5)).schur_scale == 0.5


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def systems():
    return {name: SR.oracle_system(builder, kw, opts) for name, builder, kw, opts in SR.SYSTEMS}


@pytest.mark.parametrize("name", [s[0] for s in SR.SYSTEMS])
def test_reference_full_is_the_oracle_and_the_variants_differ(systems, name):
    spec, u0, u, o, J, F = systems[name]
    x = np.random.default_rng(11).standard_normal(J.shape[1:2] + J.shape[3:])
    SR.check_full_is_oracle(o.pc, x)
    y = {f: SR.stage1_fact(o.pc, x, f) for f in SR.FACTS}
    # the identities that tell the variants apart, all bitwise in the reference
    r0, r1 = SR.stage1_rhs(o.pc, x)
    assert np.array_equal(y["lower"][1], y["full"][1]) and np.array_equal(y["lower"][0], o.pc.amg_p.vcycle(r0))
    assert np.array_equal(y["upper"][1], SR.ks_of(o.pc)(r1)) and np.array_equal(y["diag"][1], -y["upper"][1])
    assert np.array_equal(y["diag"][0], y["lower"][0])
    assert np.array_equal(SR.stage1_fact(o.pc, x, "diag", 0.5)[1], 0.5*y["upper"][1])
    assert not np.array_equal(y["lower"][0], y["full"][0]) and not np.array_equal(y["upper"][1], y["full"][1])
    assert all(not y[f][2:].any() for f in SR.FACTS)


@pytest.mark.parametrize("name", [s[0] for s in SR.SYSTEMS])
@pytest.mark.parametrize("fact", SR.FACTS)
def test_oracle_fgmres_converges_with_the_recorded_counts(systems, name, fact):
    spec, u0, u, o, J, F = systems[name]
    d, its, reason = SR.fgmres_fact(o, J, F, fact)
    assert reason == 2
    assert its == SR.COUNTS[name][SR.FACTS.index(fact)]
    assert np.linalg.norm(F - SR.la.spmv_block(J, d)) <= 1.01*o.opts["ksp_rtol"]*np.linalg.norm(F)
