"""The composite's temperature stage (pc_ctr): what can be checked without a GPU -- the option through every
layer, the refusals, the PETSc spelling of the trailing temperature-only entry, and the numpy reference tests/ctr_ref.py on the
small single-phase system the GPU tests use (tests/test_gpu_ctr.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import ctr_ref as CR
import pc_order_ref as PR
from optpack import differing_fields
from thermalporous_amd.engine import API_SYMBOLS, DEFAULT_OPTS, HipEngine, check_pc_ctr_options, tp_options
from thermalporous_amd.solver_options import engine_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "thermalporous_hip.h")


# ---- options ------------------------------------------------------------------------------------------------------------------
def test_default_struct_field_header_and_exports():
    assert DEFAULT_OPTS["pc_ctr"] is False
    names = [f[0] for f in tp_options._fields_]
    assert dict(tp_options._fields_)["pc_ctr"] is C.c_int32
    i = names.index("pc_ctr")
    assert names[i - 1] == "ilu_levels" and names[i + 1] == "fs_additive"
    text = open(HEADER).read()
    assert "int32_t pc_ctr;" in text
    assert text.index("int32_t ilu_levels;") < text.index("int32_t pc_ctr;") < text.index("int32_t fs_additive;")
    for decl in ("int tp_ctr_rhs(tp_ctx *ctx, int32_t x, int32_t y, int32_t out);", "int tp_ctr_apply(tp_ctx *ctx, int32_t x, int32_t y);",
                 "int tp_ctr_info(tp_ctx *ctx, int32_t out[4]);"):
        assert decl in text
    assert {"tp_ctr_rhs", "tp_ctr_apply", "tp_ctr_info"} <= set(API_SYMBOLS)
    for name in ("ctr_rhs", "ctr_apply", "ctr_info"):
        assert callable(getattr(HipEngine, name))


def test_struct_is_byte_identical_without_the_key_in_every_other_field():
    base = dict(DEFAULT_OPTS, ilu_tile=(1 << 30, 8, 8))
    base.pop("pc_ctr")
    a = HipEngine._make_options(base)                       # without the key
    assert a.pc_ctr == 0
    for v, code in ((False, 0), (True, 1)):
        b = HipEngine._make_options(dict(base, pc_ctr=v))
        assert b.pc_ctr == code
        assert differing_fields(a, b) <= {"pc_ctr"}


def test_refusals_name_both_options():
    for pc in ("cptramg", "fieldsplit_cd", "bilu"):
        with pytest.raises(NotImplementedError, match=r"pc_ctr.*%s" % pc):
            check_pc_ctr_options(dict(DEFAULT_OPTS, pc=pc, pc_ctr=True))
        check_pc_ctr_options(dict(DEFAULT_OPTS, pc=pc))                                  # off goes with every kind
    for nranks in (2, 3):
        with pytest.raises(NotImplementedError, match=r"pc_ctr.*nranks = %d" % nranks):
            check_pc_ctr_options(dict(DEFAULT_OPTS, pc_ctr=True), nranks)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="pc_ctr"):
            check_pc_ctr_options(dict(DEFAULT_OPTS, pc_ctr=bad))
    # allowed: cpr and cptr, every decoupling, both ILU levels, every order
    for pc in ("cpr", "cptr"):
        for extra in ({}, {"decoup": "QI"}, {"decoup": "TI"}, {"ilu_levels": 1}, {"pc_order": "ISI"}, {"pc_order": "SIS"}):
            check_pc_ctr_options(dict(DEFAULT_OPTS, pc=pc, pc_ctr=True, **extra))
    # through the PETSc dicts, with the build key
    with pytest.raises(NotImplementedError, match=r"pc_ctr.*bilu"):
        engine_options({"snes_type": "newtonls", "ksp_type": "fgmres", "mat_type": "aij", "pc_type": "bjacobi", "sub_pc_type": "ilu",
                        "pc_ctr": True}, "Two-phase")


# ---- the PETSc spelling --------------------------------------------------------------------------------------------------------
V = {"ksp_type": "preonly", "pc_type": "hypre", "pc_hypre_type": "boomeramg", "pc_hypre_boomeramg_max_iter": 1}
BASE = {"snes_type": "newtonls", "ksp_type": "fgmres", "mat_type": "aij", "pc_type": "composite", "pc_composite_type": "multiplicative"}


def split_entry(k, f0, f1):
    """An additive fieldsplit entry: one V-cycle on the fields f0, zero on the fields f1 (gmres, max_it 0, pc none)."""
    p = "sub_%d_" % k
    d = {p + "pc_fieldsplit_type": "additive", p + "pc_fieldsplit_0_fields": f0, p + "fieldsplit_0": dict(V),
         p + "fieldsplit_1_ksp_type": "gmres", p + "fieldsplit_1_ksp_max_it": 0, p + "fieldsplit_1_pc_type": "none"}
    if f1 is not None:
        d[p + "pc_fieldsplit_1_fields"] = f1
    return d


def python_entry(k, decoup):
    return {"sub_%d_pc_python_type" % k: "thermalporous.preconditioners.CPRStage1PC", "sub_%d_cpr_stage1" % k: dict(V),
            "sub_%d_cpr_decoup" % k: decoup}


def ilu_entry(k):
    return {"sub_%d_sub_pc_type" % k: "ilu", "sub_%d_sub_pc_factor_levels" % k: 0}


def ctr_dict(first="fieldsplit", two_phase=True, rest="default", key=True):
    """X, bjacobi, T: the three-entry composite of the reference's cprctr_gmres, written from its description."""
    others = "0,2" if two_phase else "0"
    d = dict(BASE, pc_composite_pcs=first + ",bjacobi,fieldsplit")
    d.update(split_entry(0, "0", "1,2" if two_phase else "1") if first == "fieldsplit" else python_entry(0, "TI"))
    d.update(ilu_entry(1))
    d.update(split_entry(2, "1", others if rest == "default" else rest))
    if key:
        d["pc_ctr"] = True
    return d


@pytest.mark.parametrize("first", ["fieldsplit", "python"])
@pytest.mark.parametrize("two_phase", [True, False], ids=["2ph", "1ph"])
def test_the_dict_is_accepted_with_the_key(first, two_phase):
    model = "Two-phase" if two_phase else "Single phase"
    o = engine_options(ctr_dict(first, two_phase), model, decoup="TI" if first == "python" else "No")
    assert (o["pc_order"], o["pc"], o["pc_ctr"]) == ("SI", "cpr", True)
    assert o["decoup"] == ("TI" if first == "python" else "No")
    # the same options as the two-entry dict, but for the key
    two = {k: v for k, v in ctr_dict(first, two_phase, key=False).items() if not k.startswith("sub_2_")}
    two["pc_composite_pcs"] = first + ",bjacobi"
    ref = engine_options(two, model, decoup="TI" if first == "python" else "No")
    assert {k: v for k, v in o.items() if k != "pc_ctr"} == {k: v for k, v in ref.items() if k != "pc_ctr"} and ref["pc_ctr"] is False
    # the remaining fields: blanks ignored, absent allowed, anything else refused
    for rest in (" 0 , 2 " if two_phase else " 0 ", None):
        assert engine_options(ctr_dict(first, two_phase, rest=rest), model, decoup=o["decoup"])["pc_ctr"] is True
    with pytest.raises(NotImplementedError, match="pc_fieldsplit_1_fields"):
        engine_options(ctr_dict(first, two_phase, rest="0" if two_phase else "0,2"), model, decoup=o["decoup"])


@pytest.mark.parametrize("first", ["fieldsplit", "python"])
def test_the_same_dict_without_the_key_is_still_refused(first):
    decoup = "TI" if first == "python" else "No"
    with pytest.raises(NotImplementedError, match=r"temperature-only stage.*not implemented.*pc_ctr: True"):
        engine_options(ctr_dict(first, key=False), "Two-phase", decoup=decoup)
    d = ctr_dict(first)
    d["pc_ctr"] = False
    with pytest.raises(NotImplementedError, match=r"temperature-only stage.*not implemented"):
        engine_options(d, "Two-phase", decoup=decoup)


def test_the_key_alone_appends_the_stage_and_other_orders_map_as_before():
    d = {k: v for k, v in ctr_dict().items() if not k.startswith("sub_2_")}
    d["pc_composite_pcs"] = "fieldsplit,bjacobi"
    o = engine_options(dict(d, pc_order="ISI"), "Two-phase")
    assert (o["pc_order"], o["pc_ctr"]) == ("ISI", True)
    # bjacobi, X, T
    d = dict(BASE, pc_composite_pcs="bjacobi, fieldsplit, fieldsplit,", pc_ctr=True)
    d.update(ilu_entry(0))
    d.update(split_entry(1, "0", "1,2"))
    d.update(split_entry(2, "1", "0,2"))
    o = engine_options(d, "Two-phase")
    assert (o["pc_order"], o["pc"], o["pc_ctr"]) == ("IS", "cpr", True)
    assert engine_options(dict(d, pc_order="IS"), "Two-phase")["pc_order"] == "IS"
    # ... together with a pc_order whose sequence the entry does not end
    with pytest.raises(NotImplementedError, match=r"pc_order.*would not end"):
        engine_options(dict(d, pc_order="ISI"), "Two-phase")


def test_refused_spellings():
    # a T entry that is not the last one
    d = dict(BASE, pc_composite_pcs="fieldsplit,fieldsplit,bjacobi", pc_ctr=True)
    d.update(split_entry(0, "0", "1,2"))
    d.update(split_entry(1, "1", "0,2"))
    d.update(ilu_entry(2))
    with pytest.raises(NotImplementedError, match="last stage only"):
        engine_options(d, "Two-phase")
    # a second T entry
    d = ctr_dict()
    d["pc_composite_pcs"] = "fieldsplit,bjacobi,fieldsplit,fieldsplit"
    d.update(split_entry(3, "1", "0,2"))
    with pytest.raises(NotImplementedError, match="pc_ctr runs one"):
        engine_options(d, "Two-phase")
    # a bogus key under the T entry
    d = ctr_dict()
    d["sub_2_bogus"] = 1
    with pytest.raises(KeyError, match="bogus"):
        engine_options(d, "Two-phase")
    # an inner Krylov in the T entry, both spellings
    d = ctr_dict()
    d["sub_2_fieldsplit_0"] = dict(V, ksp_type="richardson", ksp_max_it=2)
    with pytest.raises(NotImplementedError, match=r"sub_2_fieldsplit_0_ksp_type.*temperature-only stage"):
        engine_options(d, "Two-phase")
    d = ctr_dict()
    d["sub_2_fieldsplit_0"] = dict(V, pc_hypre_boomeramg_max_iter=2)
    with pytest.raises(NotImplementedError, match=r"sub_2_fieldsplit_0_pc_hypre_boomeramg_max_iter.*temperature-only stage"):
        engine_options(d, "Two-phase")
    # a second split that is not "returns zero", and a split type other than additive
    d = ctr_dict()
    d["sub_2_fieldsplit_1_ksp_max_it"] = 1
    with pytest.raises(NotImplementedError, match="sub_2_"):
        engine_options(d, "Two-phase")
    d = ctr_dict()
    d["sub_2_pc_fieldsplit_type"] = "multiplicative"
    with pytest.raises(NotImplementedError, match="sub_2_pc_fieldsplit_type"):
        engine_options(d, "Two-phase")


# ---- the reference ----------------------------------------------------------------------------------------------------------
def test_reference_alone_reproduces_the_recorded_counts():
    """The 14 x 19 single-phase system: apply_seq("SI") IS TwoStagePC.apply bit for bit, and the oracle FGMRES converges under SI,
    SIT, IST, ISIT, SIST after 4, 2, 2, 2, 2 iterations with reason 2."""
    name, builder, kw, opts = CR.TABLE[0]
    spec, u0, u, o, J, F = PR.oracle_system(builder, kw, opts)
    amgT = CR.make_ctr_amg(o.pc)
    x = np.random.default_rng(11).standard_normal(J.shape[1:2] + J.shape[3:])
    assert np.array_equal(CR.apply_seq(o.pc, amgT, "SI", x), o.pc.apply(x))
    got = []
    for seq in ("SI",) + CR.SEQS:
        d, its, reason = CR.fgmres_seq(o, amgT, J, F, seq)
        assert reason == 2, seq
        got.append(its)
    assert tuple(got) == tuple(CR.count(name, s) for s in ("SI",) + CR.SEQS) == (4, 2, 2, 2, 2)
    # the pieces: with y = 0 the row right-hand side is x_T itself; the stage alone has zero fields but T
    assert np.array_equal(CR.row_rhs_ref(o.pc, x, np.zeros_like(x)), x[1])
    y = CR.ctr_apply_ref(amgT, x)
    assert np.array_equal(y[1], amgT.vcycle(x[1])) and not y[0].any()
