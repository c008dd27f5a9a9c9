"""The Python-visible surface of the extension module `_CXX_i8ie`, pinned whole: for the module and for every class in it,
the sorted public attribute names (plus `__init__` and `__call__`, which carry overloads) and every callable's `__doc__`.
pybind11 writes each overload's signature into `__doc__` in registration order, with argument names and defaults, and it
tries overloads in that order: the dump is the names, the signatures and the overload order at once.  Importing the module
creates no device context, so this needs no GPU.

tests/golden/binding_surface.json was written by this file's `__main__` from a build of the commit before the binding was
split into csrc/binding/; equality is exact.

usage:  python tests/test_binding_surface.py      (rewrites the golden from the extension as built)
"""
import inspect
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "binding_surface.json")
SPECIAL = ("__init__", "__call__")


def _names(obj):
    return sorted(n for n in dir(obj) if not n.startswith("_") or (n in SPECIAL and inspect.isclass(obj)))


def _members(obj):
    out = {}
    for n in _names(obj):
        v = getattr(obj, n)
        if inspect.isclass(v):
            continue
        out[n] = v.__doc__ if callable(v) else repr(v)
    return out


def dump_surface():
    import int8inferenceengine_amd  # noqa: F401  (puts _CXX_i8ie on the path)
    import _CXX_i8ie as cx

    classes = {n: getattr(cx, n) for n in _names(cx) if inspect.isclass(getattr(cx, n))}
    return {
        "doc": cx.__doc__,
        "names": _names(cx),
        "functions": _members(cx),
        "classes": {n: {"doc": c.__doc__, "bases": [b.__name__ for b in c.__mro__[1:]], "names": _names(c), "members": _members(c)}
                    for n, c in classes.items()},
    }


def test_surface_is_the_recorded_one():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(dump_surface()))
    assert sorted(got["classes"]) == sorted(want["classes"])
    assert got["names"] == want["names"]
    for n in want["functions"]:
        assert got["functions"][n] == want["functions"][n], n
    for cn, c in want["classes"].items():
        assert got["classes"][cn]["names"] == c["names"], cn
        for n in c["members"]:
            assert got["classes"][cn]["members"][n] == c["members"][n], "%s.%s" % (cn, n)
    assert got == want


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.dirname(HERE))
    with open(GOLDEN, "w") as f:
        json.dump(dump_surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
