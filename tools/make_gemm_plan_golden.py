"""Record tests/golden/gemm_plan_table.json: what st_gemm_plan answers for every descriptor of tests/_gemm_plan_cases.py -- one row per case,
[name, 1 (accepted) or 0 (ST_EINVAL), the four plan values or null].  st_gemm_plan is the only entry called: it launches nothing and follows no
pointer, so the made-up addresses of the cases are safe with or without a GPU.  The table is meant to change only with a deliberate change of the
dispatch; a refactor must reproduce it (tests/test_gemm_plan_cpu.py).
usage: python tools/make_gemm_plan_golden.py [out.json]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def table(plan_fn=None):
    """rows for every case; plan_fn(desc0, desc1 or None) -> (rc, [4 ints]) defaults to st_gemm_plan"""
    import _gemm_plan_cases as cases
    if plan_fn is None:
        from stitch_amd._lib import lib

        def plan_fn(d0, d1):
            p = (C.c_int32 * 4)()
            rc = lib.st_gemm_plan(C.byref(d0), C.byref(d1) if d1 is not None else None, p)
            return rc, list(p)
    rows = []
    for name, _tags, f0, f1 in cases.CASES:
        rc, plan = plan_fn(cases.desc(f0), cases.desc(f1) if f1 is not None else None)
        assert rc in (0, 1001), (name, rc)
        rows.append([name, int(rc == 0), plan if rc == 0 else None])
    return rows


def dump(rows, path):
    with open(path, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")


if __name__ == "__main__":
    import stitch_amd  # noqa: F401  (puts the package on the path under its import name)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "gemm_plan_table.json")
    rows = table()
    dump(rows, out)
    print(f"{len(rows)} rows, {sum(r[1] for r in rows)} accepted -> {out}")
