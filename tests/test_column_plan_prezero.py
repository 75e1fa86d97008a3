"""
``ColumnPlan::accepts_prezeroed`` of ``slmsuite_amd/csrc/column_plan.hpp`` without a GPU: whether the row launch ahead of a body
may store the zero H of the empty columns instead of their G (``RowArgs::zero_mask``) and the body's column launch may walk past
empty half tiles (``ColArgs::h_prezeroed``).  ``tests/column_plan_host.cpp`` forms the facts of a cfg-2-like body and plans it with
``plan_column_pass``; the table below names every fact that must turn the field off.
"""
import pytest

from plan_host import GS, KIM, LEONARDO, NOGRETTE, host, plan  # noqa: F401  (host: the fixture)


def _ask(exe, **facts):
    p = plan(exe, preset="cfg2", **facts)
    main = p["main"]
    return dict(ok=p["accepts_prezeroed"], family=main["family"] if main["family"] == "tile2" else "other", col_flags=main["col_flags"],
                phase_mode=main["phase_mode"])


def test_true_for_the_headline_and_the_batch(host):
    """cfg 2 (one hologram, 32 active columns of 4096, column lists off) and cfg 3 (a batch of eight): bodies with and without a
    weight update, GS as well."""
    for batch in (1, 8):
        for method, upd in ((LEONARDO, 1), (LEONARDO, 0), (GS, 0), (KIM, 0)):
            got = _ask(host, B=batch, method=method, do_update=upd)
            assert got == dict(ok=1, family="tile2", col_flags=1, phase_mode=0), (batch, method, upd, got)
    # (a quarter of the columns active is the most the flags go with)
    assert _ask(host, n_active=1024)["ok"] == 1
    assert _ask(host, n_active=1025)["ok"] == 0


FALSE_CASES = {
    "loads off": dict(HGS_OPT_EMPTY_COL_LOADS=0),
    "inverse off": dict(HGS_OPT_EMPTY_COL_INVERSE=0),
    "forward off": dict(HGS_OPT_EMPTY_COL_FORWARD=0),
    "prezero off": dict(HGS_OPT_EMPTY_COL_PREZERO=0),
    "PHASE 1 (WGS-Kim stores the farfield phase)": dict(method=KIM, store_phase=1),
    "PHASE 2 (WGS-Kim reads it)": dict(method=KIM, use_fixed=1),
    "2048 rows": dict(Ph=2048, Sh=520),
    "six slots": dict(Sh=1500),
    "a weight written outside the scan": dict(w_outside_scan=1),
    "a dirty scan": dict(sparse_dirty=1),
    "a dirty scan that counted nothing": dict(sparse_dirty=1, n_active=0),
    "MRAF": dict(mraf=1),
    "MRAF, normalised weights (pre-sum form)": dict(mraf=1, w_unit=1),
    "MRAF without an update": dict(mraf=1, do_update=0),
    "statistics": dict(stat_groups=1),
    "spot statistics": dict(stat_groups=2),
    "Nogrette": dict(method=NOGRETTE),
    "fp64": dict(elem=8),
    "column lists": dict(sparse_enabled=1, HGS_OPT_SPARSE_COLUMNS=1),
    "half-width kernel off": dict(HGS_TILE2=0),
    "8192 rows": dict(Ph=8192, Pw=8192, Sh=2304),
}


@pytest.mark.parametrize("why", sorted(FALSE_CASES))
def test_false(host, why):
    for batch in (1, 8):
        got = _ask(host, B=batch, **FALSE_CASES[why])
        assert got["ok"] == 0, (why, batch, got)


def test_the_switch_alone_changes_no_plan(host):
    """HGS_OPT_EMPTY_COL_PREZERO off: the same main launch, only the predicate turns."""
    on, off = _ask(host), _ask(host, HGS_OPT_EMPTY_COL_PREZERO=0)
    assert on["ok"] == 1 and off["ok"] == 0
    assert {k: v for k, v in on.items() if k != "ok"} == {k: v for k, v in off.items() if k != "ok"}
    # ... in every field of the plan; only the row launch ahead of such a body stops storing the zeros
    on, off = plan(host, preset="cfg2"), plan(host, preset="cfg2", HGS_OPT_EMPTY_COL_PREZERO=0)
    assert on["close_next"]["zero_par"] >= 0 and off["close_next"]["zero_par"] == -1
    off["accepts_prezeroed"], off["close_next"]["zero_par"] = on["accepts_prezeroed"], on["close_next"]["zero_par"]
    assert on == off
