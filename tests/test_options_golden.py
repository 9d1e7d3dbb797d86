"""The option plumbing against tests/golden/options_golden.json (made by tests/golden/make_options_golden.py at the commit named
in the file, before the plumbing was rewritten): the bytes HipEngine._make_options packs, and what engine_options makes of the
presets and of dicts that say an option twice -- the options, or the exception's type and message.  No GPU needed."""
import json
import os

import pytest

from optpack import expand, field_bytes, patched
from thermalporous_amd.engine import HipEngine, tp_options
from thermalporous_amd.solver_options import engine_options

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "options_golden.json")))
# the file stores every dict as a change of another one, the packed bytes as the fields that differ from the first case's
PACK = [(expand(GOLDEN["defaults"], c), patched(bytes.fromhex(GOLDEN["pack"][0]["hex"]), tp_options, c.get("fields", {})))
        for c in GOLDEN["pack"]]
SP = []
for c in GOLDEN["map"]:
    SP.append(expand({} if c["like"] is None else SP[c["like"]], c))


def lists(v):
    """Tuples as lists, all the way down (JSON has no tuples)."""
    if isinstance(v, dict):
        return {k: lists(x) for k, x in v.items()}
    return [lists(x) for x in v] if isinstance(v, (list, tuple)) else v


def test_every_recorded_dict_packs_to_the_recorded_bytes():
    assert len(PACK[0][1]) == len(bytes(tp_options()))
    for opts, packed in PACK:
        assert bytes(HipEngine._make_options(opts)) == packed, opts


def test_the_corpus_varies_every_field():
    """At every field's offset at least two different values occur, so no slot mix-up can hide behind a field never varied."""
    structs = [tp_options.from_buffer_copy(packed) for _, packed in PACK]
    for name, *_ in tp_options._fields_:
        assert len({field_bytes(t, name) for t in structs}) >= 2, name


@pytest.mark.parametrize("i", range(len(SP)), ids=["%02d %s" % (i, c["name"]) for i, c in enumerate(GOLDEN["map"])])
def test_solver_parameters_map_as_recorded(i):
    case = GOLDEN["map"][i]
    want = case["out"] if isinstance(case["out"], list) else expand(GOLDEN["defaults"], case["out"])
    try:
        out = lists(engine_options(SP[i], case["model"], case["decoup"], case["vector"]))
    except (NotImplementedError, ValueError, KeyError) as e:
        out = [type(e).__name__, e.args[0]]
    assert out == want and json.dumps(out, sort_keys=True) == json.dumps(want, sort_keys=True)
