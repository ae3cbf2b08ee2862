"""Regenerate tests/golden/first_solvers_cases_expected.json: (niter, status) of every case of tests/first_solvers_cases.py on the
CPU oracle as committed.  niter is null where the case does not qualify for history parity (the oracle's two dot modes disagree).
The endings the table is named for are pinned by hand in tests/test_first_solvers_cases_host.py, not from this file.

    python tests/golden/make_first_solvers_cases.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import oracle as ok  # noqa: E402
import first_solvers_cases as fc  # noqa: E402

ok.lib()
rows = []
for s in fc.SOLVERS:
    one = []
    for name in fc.CASES[s]:
        r = fc.oracle_run(ok, s, name)
        q, _ = fc.qualifies(ok, s, name)
        one.append("  %s: %s" % (json.dumps(name), json.dumps([r.niter if q else None, r.status], ensure_ascii=False)))
    rows.append(' "%s": {\n' % s + ",\n".join(one) + "\n }")
with open(os.path.join(HERE, "first_solvers_cases_expected.json"), "w", encoding="utf-8") as f:
    f.write("{\n" + ",\n".join(rows) + "\n}\n")
