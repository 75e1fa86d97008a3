"""
The walk over the scan's tile list and the two predicates that go with it, without a GPU.

``tile2_next_listed`` of ``slmsuite_amd/csrc/tile_flags.hpp`` is plain C++ that ``col_tile2_kernel`` instantiates with scalar
loads of the list and of the flag words (``ColArgs::tile_list``).  ``tests/tile_list_host.cpp`` plays it for every workgroup of
grids of 2 - 16 workgroups over every flag row of 1 - 5 tiles, every empty / non-empty pattern of six, and random rows of 64,
and compares with the flag words and with the static walk (``tile2_next_nonempty``); it is built as the stand-alone program
it is, with AddressSanitizer and UndefinedBehaviorSanitizer.  Nothing is loaded into Python.

``ColLaunch::wslots`` (which launches leave their weight-norm partials per half tile) and ``EmptyCols::list_walk`` (which walk the
list where the row launch before left the zeros) of ``column_plan.hpp`` are read from the plan ``tests/column_plan_host.cpp``
prints, on the cases ``test_column_plan_prezero.py`` asks ``accepts_prezeroed``.
"""
import os
import subprocess

import pytest

from plan_host import CSRC, GS, KIM, LEONARDO, NOGRETTE, build, host, plan  # noqa: F401  (host: the fixture)


@pytest.fixture(scope="module")
def walk_host(tmp_path_factory):
    return build(tmp_path_factory, "tile_list_host", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def test_list_walk_visits_every_non_empty_half_tile_once(walk_host):
    r = subprocess.run([walk_host], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[0] == "checked" and int(tail[3]) == 0, r.stdout[-2000:]
    # 9 grids x (16 + .. + 16^5 rows + 4096 + 3004)
    assert int(tail[1]) == 9 * (sum(16 ** n for n in range(1, 6)) + 4096 + 3004), r.stdout[-200:]


def test_kernel_walks_the_list_through_the_helper_only():
    """col_tile2_kernel finds its list positions through the helper, fed by scalar loads: no second spelling of the walk, and the
    header stays host-callable."""
    src = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert src.count("tile2_next_listed(list_at, flag_word, &pos, ct_step, nlist, ntiles, half") == 2
    assert "auto list_at = [&](int p) { return uniform_load_i32(tlist + p); };" in src
    assert "tile2_listed(word[t])" in src          # (the device kernel that writes the list asks the same predicate)
    hdr = open(os.path.join(CSRC, "tile_flags.hpp")).read()
    assert "hip/" not in hdr and "__global__" not in hdr


def _ask(exe, **facts):
    """The cfg-2-like body behind a row launch that left the zeros wherever the body accepts them (the engine never leaves them
    ahead of another): whether it leaves slots, walks the list, accepts the zeros."""
    p = plan(exe, preset="cfg2", **facts)
    if p["accepts_prezeroed"]:
        p = plan(exe, preset="cfg2", gh_prezeroed=1, **facts)
    main = p["main"]
    assert main["empty"]["prezeroed"] == p["accepts_prezeroed"]
    return dict(slots=main["wslots"], list=main["empty"]["list_walk"], prezero=p["accepts_prezeroed"],
                family=main["family"] if main["family"] == "tile2" else "other", col_flags=main["col_flags"], few=main["few_active"], grid=main["grid"])


def test_slots_and_list_for_the_headline_and_the_batch(host):
    """cfg 2 and cfg 3: an updating body leaves slots and walks the list; a body without an update walks the list and leaves no
    partial at all.  The grid stays the planned one."""
    for batch, grid in ((1, 768), (8, 96)):
        got = _ask(host, B=batch)
        assert got == dict(slots=1, list=1, prezero=1, family="tile2", col_flags=1, few=1, grid=grid), (batch, got)
        for method, upd in ((LEONARDO, 0), (GS, 0), (KIM, 0)):
            got = _ask(host, B=batch, method=method, do_update=upd)
            assert (got["slots"], got["list"], got["prezero"], got["grid"]) == (0, 1, 1, grid), (batch, method, got)


# every accepts_prezeroed case: (facts, main.wslots, main.empty.list_walk, accepts_prezeroed)
CASES = {
    "list off": (dict(HGS_OPT_EMPTY_COL_LIST=0), 1, 0, 1),
    "prezero off": (dict(HGS_OPT_EMPTY_COL_PREZERO=0), 1, 0, 0),
    "forward off": (dict(HGS_OPT_EMPTY_COL_FORWARD=0), 1, 0, 0),
    "inverse off": (dict(HGS_OPT_EMPTY_COL_INVERSE=0), 1, 0, 0),
    # no flags go with the launch, the instance (few active columns -> NXF) is the same: slots, written for every half tile
    "loads off": (dict(HGS_OPT_EMPTY_COL_LOADS=0), 1, 0, 0),
    "weight written behind the scan": (dict(w_outside_scan=1), 1, 0, 0),
    # one hologram with many active columns runs the parked form without NXF, which keeps the per-workgroup partial ...
    "many active columns": (dict(n_active=1025), 0, 0, 0),
    "scan not current": (dict(sparse_dirty=1), 0, 0, 0),
    # ... a batch runs the register form whatever the columns hold: slots with and without flags
    "batch, many active columns": (dict(B=8, n_active=1025), 1, 0, 0),
    "batch, scan not current": (dict(B=8, sparse_dirty=1), 1, 0, 0),
    "batch, loads off": (dict(B=8, HGS_OPT_EMPTY_COL_LOADS=0), 1, 0, 0),
    "six slots": (dict(Sh=1300), 0, 0, 0),
    "batch, six slots": (dict(B=8, Sh=1300), 0, 0, 0),
    "2048 rows": (dict(Ph=2048, Sh=1080), 0, 0, 0),
    "8192 rows": (dict(Ph=8192), 0, 0, 0),
    "float64": (dict(elem=8), 0, 0, 0),
    "phase stored": (dict(method=KIM, store_phase=1), 0, 0, 0),
    "phase read": (dict(method=KIM, use_fixed=1), 0, 0, 0),
    "half-width kernel off": (dict(HGS_TILE2=0), 0, 0, 0),
    "MRAF": (dict(mraf=1), 0, 0, 0),
    "statistics": (dict(stat_groups=1), 0, 0, 0),
    "Nogrette": (dict(method=NOGRETTE), 0, 0, 0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_predicates(host, name):
    facts, slots, listed, prezero = CASES[name]
    got = _ask(host, **facts)
    assert (got["slots"], got["list"], got["prezero"]) == (slots, listed, prezero), (name, got)
    assert got["list"] <= got["prezero"]            # the list never acts without the pre-zeroed H
    if got["slots"]:
        assert got["family"] == "tile2"


def test_grid_override_changes_neither_predicate(host):
    """HGS_TILE2_BLOCKS moves the grid and nothing else: the slots make the result independent of it."""
    for blocks, grid in ((16, 16), (528, 528), (752, 752), (0, 768)):
        got = _ask(host, HGS_TILE2_BLOCKS=blocks)
        assert (got["slots"], got["list"], got["prezero"], got["grid"]) == (1, 1, 1, grid), (blocks, got)
