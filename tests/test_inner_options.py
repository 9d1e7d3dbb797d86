"""Options of the inner stage-1 solve (s1_ksp, s1_max_it, s1_rtol, s1_atol): every PETSc spelling maps to the engine options,
what is not implemented is rejected with a reason, and the C struct carries the new fields.  No GPU needed."""
import ctypes as C

import pytest

from oracle.engine import OracleEngine
from thermalporous_amd.engine import DEFAULT_OPTS, HipEngine, tp_options
from thermalporous_amd.homogeneousgeo import HomogeneousGeo
from thermalporous_amd.physicalparameters import PhysicalParameters
from thermalporous_amd.singlephase import SinglePhase
from thermalporous_amd.solver_options import _flatten, engine_options
from thermalporous_amd.twophase import TwoPhase
from thermalporous_amd.wellcase import WellCase


def preset(name, two_phase):
    """The flat PETSc dict of a string preset, as the model classes build it."""
    p = PhysicalParameters()
    if two_phase:
        p.S_o = 0.9
    g = HomogeneousGeo(8, 8, p, 20., 20.)
    c = WellCase(p, g, well_case="test0", constant_rate=True)
    cls = TwoPhase if two_phase else SinglePhase
    m = cls(g, c, p, solver_parameters=name, filename=None, verbosity=False, _engine_factory=OracleEngine)
    return _flatten(dict(m.solver_parameters)), m.name, m.decoup, bool(getattr(m, "vector", False))


def s1(o):
    return (o["s1_ksp"], o["s1_max_it"], o["s1_rtol"], o["s1_atol"])


# (preset, two-phase, prefix of the pressure / system solver)
PLACES = [("pc_cpr", False, "sub_0_cpr_stage1_"), ("pc_cpr_QI", True, "sub_0_cpr_stage1_"),
          ("pc_cptr", True, "sub_0_cpr_stage1_fieldsplit_0_"), ("pc_cptr_a11", True, "sub_0_cpr_stage1_fieldsplit_0_"),
          ("pc_cptramg_QI", True, "sub_0_cpr_stage1_"),
          ("pc_fieldsplit_cd", False, "fieldsplit_0_"), ("pc_fieldsplit_a11", False, "fieldsplit_0_"),
          ("pc_fieldsplit_selfp", False, "fieldsplit_0_"), ("pc_fieldsplit_diag", False, "fieldsplit_0_"),
          ("pc_cpr_gmres", False, "sub_0_fieldsplit_0_"), ("pc_cptr_gmres", True, "sub_0_fieldsplit_0_fieldsplit_0_")]


@pytest.mark.parametrize("name,two,prefix", PLACES, ids=[p[0] for p in PLACES])
def test_every_spelling_maps_to_engine_options(name, two, prefix):
    sp, model, decoup, vector = preset(name, two)
    eo = lambda d: engine_options(d, model, decoup, vector=vector)
    base = eo(sp)
    assert s1(base) == ("preonly", 1, 0.0, 0.0) == tuple(DEFAULT_OPTS[k] for k in ("s1_ksp", "s1_max_it", "s1_rtol", "s1_atol"))
    # k V-cycles: hypre's own iteration count, or richardson
    o = eo({**sp, prefix + "pc_hypre_boomeramg_max_iter": 3})
    assert s1(o) == ("richardson", 3, 0.0, 0.0)
    assert {k: v for k, v in o.items() if not k.startswith("s1_")} == {k: v for k, v in base.items() if not k.startswith("s1_")}
    assert s1(eo({**sp, prefix + "ksp_type": "richardson", prefix + "ksp_max_it": 2})) == ("richardson", 2, 0.0, 0.0)
    assert s1(eo({**sp, prefix + "ksp_type": "richardson", prefix + "ksp_max_it": 40})) == ("richardson", 40, 0.0, 0.0)
    # GMRES(k), right-preconditioned; tolerances given or PETSc's KSP defaults
    o = eo({**sp, prefix + "ksp_type": "fgmres", prefix + "ksp_max_it": 4, prefix + "ksp_rtol": 1e-2})
    assert s1(o) == ("fgmres", 4, 1e-2, 1e-50)
    o = eo({**sp, prefix + "ksp_type": "gmres", prefix + "ksp_pc_side": "right", prefix + "ksp_max_it": 32,
            prefix + "ksp_rtol": 1e-8, prefix + "ksp_atol": 1e-30})
    assert s1(o) == ("fgmres", 32, 1e-8, 1e-30)
    assert s1(eo({**sp, prefix + "ksp_type": "fgmres", prefix + "ksp_max_it": 1})) == ("fgmres", 1, 1e-5, 1e-50)
    # rejections
    with pytest.raises(NotImplementedError, match="LEFT"):
        eo({**sp, prefix + "ksp_type": "gmres", prefix + "ksp_max_it": 4})
    with pytest.raises(NotImplementedError):
        eo({**sp, prefix + "ksp_type": "fgmres", prefix + "ksp_max_it": 33})
    with pytest.raises(ValueError):
        eo({**sp, prefix + "ksp_type": "fgmres", prefix + "ksp_max_it": 0})
    with pytest.raises(ValueError):
        eo({**sp, prefix + "pc_hypre_boomeramg_max_iter": 0})
    with pytest.raises(NotImplementedError):
        eo({**sp, prefix + "ksp_type": "cg", prefix + "ksp_max_it": 4})
    with pytest.raises(NotImplementedError):          # the count is part of the arithmetic: it must be stated
        eo({**sp, prefix + "ksp_type": "fgmres"})
    with pytest.raises(NotImplementedError):          # hypre tuning still does not apply
        eo({**sp, prefix + "ksp_type": "fgmres", prefix + "ksp_max_it": 4, prefix + "pc_hypre_boomeramg_strong_threshold": 0.5})
    with pytest.raises(KeyError):                     # a tolerance richardson would silently ignore
        eo({**sp, prefix + "ksp_type": "richardson", prefix + "ksp_max_it": 2, prefix + "ksp_rtol": 1e-3})
    # build keys next to amg_omega combine with a preset
    o = eo({**sp, "s1_ksp": "fgmres", "s1_max_it": 4, "s1_rtol": 1e-2})
    assert s1(o) == ("fgmres", 4, 1e-2, 0.0)
    with pytest.raises(NotImplementedError):
        eo({**sp, "s1_ksp": "fgmres", "s1_max_it": 33})
    with pytest.raises(ValueError):
        eo({**sp, "s1_ksp": "richardson", "s1_max_it": 0})
    with pytest.raises(NotImplementedError):
        eo({**sp, "s1_ksp": "bicg"})
    with pytest.raises(ValueError):                   # said twice, differently
        eo({**sp, "s1_ksp": "fgmres", "s1_max_it": 4, prefix + "pc_hypre_boomeramg_max_iter": 2})


@pytest.mark.parametrize("name,two", [("pc_cpr", False), ("pc_cpr", True), ("pc_cptramg", True)])
def test_pc_ksp_spelling_of_the_python_stage(name, two):
    """CPRStage1PC / CPTRStage1PC hold a PC, so PETSc wants pc_type ksp and the solver under <prefix>ksp_."""
    sp, model, decoup, vector = preset(name, two)
    base = "sub_0_cpr_stage1_"
    moved = {k: v for k, v in sp.items() if not k.startswith(base)}
    inner = {base + "ksp_" + k[len(base):]: v for k, v in sp.items() if k.startswith(base) and k != base + "ksp_type"}
    d = {**moved, **inner, base + "pc_type": "ksp", base + "ksp_ksp_type": "fgmres", base + "ksp_ksp_max_it": 6,
         base + "ksp_ksp_rtol": 1e-3}
    o = engine_options(d, model, decoup, vector=vector)
    assert s1(o) == ("fgmres", 6, 1e-3, 1e-50) and o["pc"] == engine_options(sp, model, decoup, vector=vector)["pc"]
    d2 = {**moved, **inner, base + "pc_type": "ksp", base + "ksp_type": "preonly", base + "ksp_ksp_type": "richardson",
          base + "ksp_ksp_max_it": 2}
    assert s1(engine_options(d2, model, decoup, vector=vector)) == ("richardson", 2, 0.0, 0.0)
    with pytest.raises(NotImplementedError, match="LEFT"):
        engine_options({**d, base + "ksp_ksp_type": "gmres"}, model, decoup, vector=vector)


def test_krylov_on_the_schur_split_says_why():
    for name, two, prefixes in (("pc_cptr", True, ["sub_0_cpr_stage1_fieldsplit_1_", "sub_0_cpr_stage1_fieldsplit_1_schur_"]),
                                ("pc_cptr_a11", True, ["sub_0_cpr_stage1_fieldsplit_1_"]),
                                ("pc_fieldsplit_cd", False, ["fieldsplit_1_", "fieldsplit_1_schur_"]),
                                ("pc_fieldsplit_a11", False, ["fieldsplit_1_"]),
                                ("pc_cptr_gmres", True, ["sub_0_fieldsplit_0_fieldsplit_1_", "sub_0_fieldsplit_0_fieldsplit_1_schur_"])):
        sp, model, decoup, vector = preset(name, two)
        for prefix in prefixes:
            for extra in ({prefix + "ksp_type": "fgmres", prefix + "ksp_max_it": 4}, {prefix + "ksp_type": "richardson", prefix + "ksp_max_it": 2}):
                with pytest.raises(NotImplementedError, match="Schur complement"):
                    engine_options({**sp, **extra}, model, decoup, vector=vector)
    # the additive split has no Schur complement: its temperature block is rejected for what it is
    sp, model, decoup, vector = preset("pc_fieldsplit_diag", False)
    for extra in ({"fieldsplit_1_ksp_type": "fgmres", "fieldsplit_1_ksp_max_it": 4}, {"fieldsplit_1_pc_hypre_boomeramg_max_iter": 2}):
        with pytest.raises(NotImplementedError, match="additive split") as ei:
            engine_options({**sp, **extra}, model, decoup, vector=vector)
        assert "Schur complement" not in str(ei.value)
    sp, model, decoup, vector = preset("pc_cptr_a11", True)
    with pytest.raises(NotImplementedError, match="Schur complement"):
        engine_options({**sp, "sub_0_cpr_stage1_fieldsplit_1_pc_hypre_boomeramg_max_iter": 2}, model, decoup, vector=vector)


def test_lu_presets_and_bilu_stay_rejected():
    p = PhysicalParameters()
    p.S_o = 0.9
    g = HomogeneousGeo(8, 8, p, 20., 20.)
    c = WellCase(p, g, well_case="test0", constant_rate=True)
    with pytest.raises(NotImplementedError):
        TwoPhase(g, c, p, solver_parameters="pc_cptrlu", filename=None, _engine_factory=OracleEngine)
    with pytest.raises(NotImplementedError):
        engine_options({"pc_type": "lu", "ksp_type": "preonly"}, "Single phase")
    sp, model, decoup, vector = preset("pc_bilu", False)
    with pytest.raises(NotImplementedError):
        engine_options({**sp, "s1_ksp": "richardson", "s1_max_it": 2}, model, decoup)
    sp, model, decoup, vector = preset("pc_cpr", False)
    with pytest.raises(NotImplementedError):
        engine_options({**sp, "sub_0_cpr_stage1_pc_type": "lu"}, model, decoup)


def test_options_struct_carries_the_new_fields_last():
    names = [f[0] for f in tp_options._fields_]
    assert names[-4:] == ["s1_ksp", "s1_max_it", "s1_rtol", "s1_atol"]
    o = HipEngine._make_options({**DEFAULT_OPTS, "ilu_tile": (1 << 30, 8, 8)})
    assert (o.s1_ksp, o.s1_max_it, o.s1_rtol, o.s1_atol) == (0, 1, 0.0, 0.0)
    o = HipEngine._make_options({**DEFAULT_OPTS, "ilu_tile": (1 << 30, 8, 8), "s1_ksp": "fgmres", "s1_max_it": 8, "s1_rtol": 1e-2,
                                 "s1_atol": 1e-30})
    assert (o.s1_ksp, o.s1_max_it, o.s1_rtol, o.s1_atol) == (2, 8, 1e-2, 1e-30)
    assert HipEngine._make_options({**DEFAULT_OPTS, "ilu_tile": (1 << 30, 8, 8), "s1_ksp": "richardson"}).s1_ksp == 1
    assert tp_options.s1_rtol.offset % C.sizeof(C.c_double) == 0


def test_facade_passes_the_inner_options_through():
    import thermalporous_amd.preconditioners as pcs

    class Rec:
        b = 2

        def __init__(self):
            self.opts = dict(DEFAULT_OPTS)
            self.calls = []

        def set_options(self, **kw):
            self.opts.update(kw)
            self.calls.append(("set_options", kw))

        def pc_setup(self):
            self.calls.append("pc_setup")

    e = Rec()
    pcs.CPRStage1PC().setUp(pcs.PC(e, {"decoup": "No", "s1_ksp": "fgmres", "s1_max_it": 4, "s1_rtol": 1e-2}))
    assert e.opts["s1_ksp"] == "fgmres" and e.opts["s1_max_it"] == 4 and e.opts["s1_rtol"] == 1e-2
    assert e.calls[-1] == "pc_setup"
    e2 = Rec()
    pcs.CPRStage1PC().setUp(pcs.PC(e2, {"decoup": "No"}))
    assert e2.calls == ["pc_setup"]                   # nothing to change: no options call, as before
