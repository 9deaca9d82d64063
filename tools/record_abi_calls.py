#!/usr/bin/env python3
"""Record what the Python layer hands to the C ABI for the host-array entries (tests/abi_calls.py: the table and the stub).

    python3 tools/record_abi_calls.py [--out tests/golden/abi_calls_host.json]

Needs no GPU. Run it on the commit whose behaviour is the expectation: tests/test_abi_calls_host.py then compares every later
tree with the committed record.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import abi_calls

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "abi_calls_host.json"))
    args = ap.parse_args()
    rec = abi_calls.record()
    rows, arrays = rec["rows"], rec["arrays"]
    line = lambda d: ",\n".join(f"{json.dumps(k)}: {json.dumps(d[k], sort_keys=True)}" for k in sorted(d))  # noqa: E731
    with open(args.out, "w") as f:  # one array, one table row per line
        f.write('{"arrays": {\n' + line(arrays) + '\n},\n"rows": {\n' + line(rows) + "\n}}\n")
    print(f"{len(rows)} rows, {sum(len(r['calls']) for r in rows.values())} library calls, {len(arrays)} arrays -> {args.out}")


if __name__ == "__main__":
    main()
