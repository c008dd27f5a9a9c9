"""Records tests/golden/create_arg_rules.json: what every layer-creating entry answers to every argument tuple of
tests/create_args.py -- (return code, i8ie_last_error() text) -- from the library that is built NOW.  Run it on a build
whose argument behaviour is the one to keep (the table pins later builds to it), never to make a failing replay pass:

    python tests/golden/make_create_arg_rules.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import abi  # noqa: E402
import create_args as ca  # noqa: E402


def main():
    lib = abi.lib()
    texts, table = [], {}
    for entry in ca.SIGNATURES:
        rows = []
        for ints, scales, ptrs in ca.grid(entry):
            rc, text = ca.call(lib, entry, ints, scales, ptrs)
            assert rc != 0, (entry, ints, scales, ptrs)
            if text not in texts:
                texts.append(text)
            rows.append([list(ints), scales, ptrs, rc, texts.index(text)])
        table[entry] = rows
    with open(os.path.join(HERE, "create_arg_rules.json"), "w") as f:
        json.dump({"texts": texts, "rows": table}, f, separators=(",", ":"))
        f.write("\n")
    print("%d rows, %d distinct texts" % (sum(len(r) for r in table.values()), len(texts)))


if __name__ == "__main__":
    main()
