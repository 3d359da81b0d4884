"""Produces tests/golden/sync_statement_costs.json: the host statement's (tests/_syncstmt.py) two-stage search of every test range of tests/_synccase.py — the cost
of every coarse and fine candidate, the picks, the result.  A rolling-shutter range costs the statement 20 s of Python per stage; the tests read the stored costs
(tests/test_sync_statement.py re-derives a sample on every run, so a statement that has moved shows).

    python tests/golden/sync_statement_costs.py        (from the repository root; a few minutes on 8 cores)
"""
import json
import multiprocessing
import os
import sys

os.environ.setdefault("OMP_NUM_THREADS", "1")      # eight workers: numpy keeps to one thread each

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(case):
    import _synccase as SC
    import _syncstmt as SS
    name, shape, mode = case
    rng, _ = SC.planted(name, shape, mode)
    r = SS.search(rng, mode, **SC.search_args(name, shape, mode))
    return SC.case_key(name, shape, mode), {k: r[k] for k in ("coarse_costs", "coarse_pick", "fine_costs", "fine_pick", "value", "cost")}


if __name__ == "__main__":
    import _synccase as SC
    cases = [(n, s, m) for s in ("gpu", "stmt", "emu") for m in (1, 0) for n in sorted(SC.CLIPS)]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        out = dict(pool.map(measure, cases, chunksize=1))
    with open(os.path.join(ROOT, "tests", "golden", "sync_statement_costs.json"), "w") as f:
        json.dump({"cases": out}, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")
