"""The GEMM dispatch table, pinned without a GPU: st_gemm_plan (the plan-only twin of st_conv_gemm / st_conv_gemm_pair, run from the same check
and plan functions) answers every descriptor of tests/_gemm_plan_cases.py as tests/golden/gemm_plan_table.json records -- accept or reject, and
family / tile / split / walk for the accepted ones.  The table was recorded when the dispatcher was refactored into check -> chunk -> plan -> launch
and compared, row by row, with what the code before that refactor did with the same descriptors; it changes only with a deliberate change of
the dispatch (tools/make_gemm_plan_golden.py).  The cases carry made-up addresses: they go to st_gemm_plan and nowhere else."""
import ctypes as C
import json
import os

import pytest

import _gemm_plan_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_table.json")


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as fh:
        return {r[0]: r for r in json.load(fh)}


def _plan(f0, f1):
    from stitch_amd._lib import lib
    p = (C.c_int32 * 4)()
    d0, d1 = cases.desc(f0), (cases.desc(f1) if f1 is not None else None)
    rc = lib.st_gemm_plan(C.byref(d0), C.byref(d1) if d1 is not None else None, p)
    return rc, list(p)


def test_every_case_plans_as_recorded(table):
    assert set(table) == {c[0] for c in cases.CASES}
    wrong = []
    for name, _tags, f0, f1 in cases.CASES:
        rc, plan = _plan(f0, f1)
        assert rc in (0, 1001), (name, rc)
        if [name, int(rc == 0), plan if rc == 0 else None] != table[name]:
            wrong.append((name, rc, plan, table[name]))
    assert not wrong, wrong


def test_plan_leaves_the_last_plan_alone_and_rejects_null():
    from stitch_amd._lib import lib
    before, after = (C.c_int32 * 4)(), (C.c_int32 * 4)()
    lib.st_gemm_last_plan(before)
    for _name, _tags, f0, f1 in cases.CASES[:60]:
        _plan(f0, f1)
    lib.st_gemm_last_plan(after)
    assert list(before) == list(after)
    assert lib.st_gemm_plan(None, None, before) == 1001
    d = cases.desc(cases.CASES[0][2])
    assert lib.st_gemm_plan(C.byref(d), None, None) == 1001


# ---- the case list cannot quietly shrink ---------------------------------------------------------------------------------------------
COMMON = ["a", "w", "c", "M", "N", "K", "kh", "kw", "K_ne_khkwCin", "Ho", "Wo", "M_mod_HoWo", "epi_aux1", "gru_aux2", "zr_c2", "zr_N_odd",
          "reserved0", "reserved1", "reserved2", "reserved3", "a2_channels_le0", "a2_channels_mod32", "a2_channels_gt_Cin", "a2_align"]
C_T = ["ct_epi", "ct_M_mod4", "ct_ld_mod4", "ct_ld_lt_M", "ct_align", "ct_split_k", "ct_reach"]
REJECTS = {       # function -> the operands of its `return ST_EINVAL`s (as they stood before the refactor; cases.UNREACHABLE lists the two no descriptor can hit)
    "conv_gemm_launch": COMMON + C_T + ["a2_batch", "ct_a_ln", "w_bytes", "chunk_batch", "chunk_split_k", "chunk_c_t", "chunk_c_planes", "chunk_units_lt1",
                                        "chunk_M_mod_unit", "a_ln_kernel", "a_ln_tile", "tile_ge20", "dma_tile_not_ok", "a2_reg_tile", "ct_reg_tile",
                                        "split_batch", "split_no_workspace", "split_workspace_small", "tile_5", "tile_11"],
    "launch_rowstream": ["slices"],
    "pair_member_prepare": COMMON + ["K_lt128", "Cin_mod32", "c_t", "a_ln", "batch", "split_k", "tile_cfg", "a_align", "w_align", "ldx_mod4", "ldw_mod4",
                                     "w_bytes", "a_bytes", "reach"],
    "split3_prepare": COMMON + C_T + ["a2_batch", "ct_a2", "ct_c_planes", "Cin_mod32", "a_ln", "split3_ne1", "a_plane_stride_le0", "w_plane_stride_le0",
                                      "a_rows_le0", "w_rows_lt_N", "a_align", "w_align", "a_plane_stride_mod8", "w_plane_stride_mod8", "batch_stride_a_mod8",
                                      "batch_stride_w_mod8", "in_rows_gt_a_rows", "batch_stride_a_neg", "batch_stride_w_neg", "batch_stride_a_mod32",
                                      "batch_stride_w_mod32", "batch_a_rows", "batch_w_rows", "a_bytes", "w_bytes", "reach"],
    "conv_gemm_split3_launch": ["tile_lt31", "tile_gt39", "kpar_split_k", "kpar_batch", "walk_a2", "walk_split_k", "split_batch", "split_no_workspace",
                                "split_workspace_small"],
    "conv_gemm_split3_pair_launch": ["desc0_fp32", "desc1_fp32", "batch", "split_k", "tile_cfg"],
    "c_planes_ok": ["reserved4", "no_f32_without_planes", "M_mod32", "ncols_odd", "col0_mod32", "col0_neg", "row0_neg", "stride_le0", "stride_mod8", "rows_le0",
                    "align", "c_t", "last_row", "extent", "via_pair", "via_split3"],
}
# threshold -> the sides that need a row (a side is "lo" / "hi" or the count / K it sits at)
THRESHOLDS = {
    "skinny_M": ["lo", "hi"], "narrow_N": ["lo", "hi"], "narrow_M": ["lo", "hi"], "tile_N32": ["lo", "hi"], "dma_K128": ["lo", "hi"],
    "rowstream_K64_M16384": ["lo", "hi"], "rowstream_M262144": ["lo", "hi"], "rowstream_N384": ["lo", "hi"], "rowstream_N384_M32768": ["lo", "hi"],
    "dma_tiles": ["255", "256", "257", "511", "512", "513"], "reg_tiles": ["255", "256", "257"], "walk_tiles": ["511", "512", "513"],
    "dma_K": ["480", "512", "992", "1024"], "K": ["511", "512", "1023", "1024"],
    "s3_ntl64_2048": ["lo", "hi"], "s3_walk_K2048": ["lo", "hi"], "s3_tiles128_256": ["lo", "hi"], "s3_ntl64_256": ["255", "256", "257"],
    "s3_kpar_K1024": ["lo", "hi"], "s3_split_K512": ["lo", "hi"], "s3_tiles_256": ["255", "256", "257"], "s3_split2_256": ["255", "256", "257"],
}


def test_the_case_list_covers_what_it_must(table):
    rows = [table[c[0]] for c in cases.CASES]
    tags = {c[0]: c[1] for c in cases.CASES}
    accepted = [r for r in rows if r[1]]
    assert 2 * len(accepted) >= len(rows), (len(accepted), len(rows))
    plans = {tuple(r[2]) for r in accepted}
    # every reportable plan: fp32 families 0, 1, 2 (tiles 1-4), 3 (tiles 12-15, walk 0 and 1), 4; a split above 1 in 2 and 3
    assert {(0, 0, 1, 0), (1, 0, 1, 0), (4, 20, 1, 1)} <= plans
    assert {(2, t, 1, 0) for t in (1, 2, 3, 4)} | {(3, t, 1, 0) for t in (12, 13, 14, 15)} | {(3, 13, 1, 1)} <= plans
    assert any(p[0] == 2 and p[2] > 1 for p in plans) and any(p[0] == 3 and p[2] > 1 for p in plans)
    # split3 tiles 31-39, a split above 1, the persistent 37; both pair plans
    assert {t for f, t, _s, _w in plans if f == 8} == set(range(31, 40))
    assert any(p[0] == 8 and p[2] > 1 for p in plans) and (8, 37, 1, 1) in plans and all(p[3] == (p[1] == 37) for p in plans if p[0] == 8 and p[3] < 2)
    assert (3, 13, 1, 3) in plans and (8, 34, 1, 3) in plans
    # both chunk forms: accepted, and really beyond one launch
    for form in ("chunk:matrix", "chunk:conv"):
        hit = [c for c in cases.CASES if form in c[1]]
        assert hit and all(table[c[0]][1] and cases.needs_chunks(c[2]) for c in hit), form
    assert not any(cases.needs_chunks(c[2]) for c in cases.CASES if c[3] is None and not c[2].get("split3") and table[c[0]][1]
                   and not any(t.startswith("chunk:") for t in c[1]))
    # one row per operand of every rejection, each the accepted base of its path with that operand violated
    assert all(table[c[0]][1] for c in cases.CASES if "base" in c[1])
    have = {t for ts in tags.values() for t in ts if t.startswith("reject:")}
    want = {f"reject:{fn}:{op}" for fn, ops in REJECTS.items() for op in ops}
    assert want <= have, sorted(want - have)
    assert not any(table[n][1] for n, ts in tags.items() if any(t.startswith("reject:") for t in ts))
    assert not {f"reject:{u}" for u in cases.UNREACHABLE} & have
    # both sides of every threshold, and the two sides answer differently somewhere
    for thr, sides in THRESHOLDS.items():
        for side in sides:
            assert any(f"thr:{thr}:{side}" in ts for ts in tags.values()), (thr, side)
        answers = {tuple(table[n][2]) for n, ts in tags.items() if any(t.startswith(f"thr:{thr}:") for t in ts) and table[n][1]}
        assert len(answers) > 1, thr
