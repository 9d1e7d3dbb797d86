"""Byte-wise comparison of ctypes structures field by field (the option tests: "every other field is what it was"), and dicts
stored as changes of other dicts (tests/golden/options_golden.json)."""
import ctypes as C
import json


def field_bytes(struct, name):
    """The bytes of field `name` of a ctypes structure."""
    f = getattr(type(struct), name)
    return bytes(C.string_at(C.addressof(struct) + f.offset, f.size))


def differing_fields(a, b):
    """The names of the fields in which two structures of one type differ."""
    assert type(a) is type(b)
    return {n for n, *_ in a._fields_ if field_bytes(a, n) != field_bytes(b, n)}


def patched(base, struct_type, fields):
    """The bytes `base` of a struct_type with the fields {name: hex} written over them."""
    out = bytearray(base)
    for name, h in fields.items():
        f = getattr(struct_type, name)
        out[f.offset:f.offset + f.size] = bytes.fromhex(h)
    return bytes(out)


def delta(new, old):
    """The JSON-able dict `new` as a change of `old`: the keys to set and, if any, the keys to drop (False, 0 and 0.0 differ)."""
    d = {"set": {k: v for k, v in new.items() if k not in old or json.dumps(old[k]) != json.dumps(v)}}
    drop = [k for k in old if k not in new]
    return dict(d, drop=drop) if drop else d


def expand(old, d):
    """The dict that delta(new, old) stands for."""
    return {**{k: v for k, v in old.items() if k not in d.get("drop", ())}, **d["set"]}
