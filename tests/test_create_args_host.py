"""The argument rules of the layer-creating entries are pinned: every row of tests/golden/create_arg_rules.json -- an entry,
an argument tuple, and the (return code, i8ie_last_error() text) an earlier build answered with -- is replayed on this
build and must answer the same.  No GPU: each call carries a NULL ctx and returns before any device call."""
import json
import os

import pytest

import abi
import create_args as ca
from conftest import GOLDEN

with open(os.path.join(GOLDEN, "create_arg_rules.json")) as _f:
    TABLE = json.load(_f)


def test_table_covers_the_grid():
    assert sorted(TABLE["rows"]) == sorted(ca.SIGNATURES)
    for entry, rows in TABLE["rows"].items():
        assert [(tuple(r[0]), r[1], r[2]) for r in rows] == ca.grid(entry), entry


@pytest.mark.parametrize("entry", sorted(ca.SIGNATURES))
def test_replay(entry):
    lib = abi.lib()
    for ints, scales, ptrs, rc, text in TABLE["rows"][entry]:
        got = ca.call(lib, entry, ints, scales, ptrs)
        assert got == (rc, TABLE["texts"][text]), (entry, dict(zip(ca.int_params(entry), ints)), scales, ptrs)
