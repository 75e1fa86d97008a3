"""
The single-inverse MRAF update (``col_presum_kernel`` + ``col_tile_kernel`` RULE 5, and the rule-free RULE 6) on sparse,
spot-like targets that put a signal pixel at every edge of the device-resident bookkeeping that steers these kernels,
against a float64 restatement of one loop body (``tests/mraf_layouts.py``) and against the split form.

The groups of ``mraf_layout`` (T = Ph / 16; rows and columns are those of the target array AS THE HOST HANDS IT OVER:
``scan_active_cols`` reads stored position i = col_pos(row, T) = (row % T) * 16 + row // T of a column and sets bit
i & 15 = row // T of ``sig_rows``; the centred transforms are folded into sign factors, nothing is rolled):

    first     column 0, rows 0, 1, T-1          first tile byte, even ``sig_rows`` half, slot 0 only
    tile_end  column 3, rows T, 4T-1            c = 3 of tile 0, odd half, slots 1 and 3, quarter 0 only
    alone     column Pw/4 + 1, rows 4T, 8T-1    the only flagged column of its tile, quarter 1 only
    straddle  columns 4k+2, 4k+3 in the box     8T-1 and 8T on both (quarters 1 and 2 in one column), two more
    last      column Pw-1, rows 12T, Ph-1       last byte of the last flag word, slots 12 and 15
    lattice   column step 5, row step 12        200 pixels inside the noise box: the ordinary case

Noise (NaN): a box around ``straddle`` and ``lattice`` with no edge a multiple of 4 (or of T), and one column elsewhere that
holds a short run of NaN and no signal (scan flags: bit 2 without bit 1).  The columns of ``first``, ``tile_end``, ``alone``
and ``last`` carry bit 1 without bit 2; most tiles are empty.

D never reaches a caller (the weights read back are normalised from the main pass's own sums), so a pre-pass that loses a
group only shifts the balance of signal and noise part in the rebuilt field: the float64 test proves ON THE REFERENCE that
each such loss moves the phase by at least ten times its bound before it compares the engine with it.

The CPU tests (no mark) tie the restatement to the float64 oracle at 256 x 256; everything measured on an MI355X is in the
docstrings below and in DESIGN.md, section 5 (``report()`` appends it to the parity report).
"""
import functools

import numpy as np
import pytest

from conftest import dispatch_of, phase_rel_l2, rel_l2, report
from mraf_layouts import GROUPS, mraf_layout, noise_only_column, reference_body, tile_slots, weights_rel_l2
from oracle import hgs_oracle as orc
from slmsuite_amd import synth

gpu = pytest.mark.gpu

MRAF = 0.5
EXPONENT = orc.ALGORITHM_DEFAULTS["WGS-Leonardo"]["feedback_exponent"]
SLMS = [(1000, 1280), (1152, 1920), (1300, 1920)]            # 4, 5 and 6 register slots at 4096 rows
PHASE_BOUND, WEIGHT_BOUND = 5e-6, 3e-6                       # one teacher-forced body (header of tests/test_gpu_parity.py)
SEED = 7


@functools.lru_cache(maxsize=None)
def layout(n, groups=GROUPS, noise_column=True):
    """Shared and left unchanged by every test."""
    t, g = mraf_layout((n, n), groups, noise_column)
    t.setflags(write=False)
    return t, g


def assert_conditioned(ref):
    """
    No signal pixel on a speckle zero (or far above its target), on the reference: |F| / (||F|| T sqrt(S / P)) within
    [0.25, 4].  The factor sqrt(S / P) (S, P = pixels of the SLM and of the padded plane) is the share of a spot's
    amplitude that its peak pixel can hold -- |F_p| <= ||F|| sqrt(S / P) for any field confined to the SLM window, and the
    peaks of isolated spots hold S / P of their power between them: without it the window [0.25, 4] asks for
    |F| / (||F|| T) >= 0.25 at every pixel where its root mean square cannot exceed sqrt(S / P) = 0.276 (4096 x 4096,
    SLM 1000 x 1280), which no hologram meets two bodies from a seed.  Measured without the factor: 0.084 .. 0.51.
    """
    r = ref["ratio"] / ref["peak"]
    assert r.min() >= 0.25 and r.max() <= 4.0, (r.min(), r.max(), ref["ratio"].min(), ref["ratio"].max())


def assert_sensitive(ref, groups, noise_only=True):
    """Every mutant of the reference -- a group lost by the pre-pass, the NaN-only column lost by the main pass -- lies at
    least ten phase bounds from the reference's own phase."""
    names = list(groups) + (["noise_only"] if noise_only else [])
    assert set(names) <= set(ref["mutants"]), (names, list(ref["mutants"]))
    dist = {g: phase_rel_l2(ref["mutants"][g], ref["phase"]) for g in names}
    assert min(dist.values()) >= 10 * PHASE_BOUND, dist
    return dist


# ---- CPU: the restatement against the oracle -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_state(n=256, slm=(96, 160)):
    t, groups = mraf_layout((n, n), GROUPS)
    o = orc.OracleHologram(t.astype(np.float64), phase=synth.seed_phase(SEED, slm, dtype=np.float64), slm_shape=slm, dtype=np.float64)
    o.optimize("WGS-Leonardo", maxiter=2, mraf_factor=MRAF, populate=False)
    ref = reference_body(o.target, groups, o.phase, o.weights, MRAF, EXPONENT)
    return o, groups, ref


def test_layout_puts_every_group_where_the_table_says():
    for n in (256, 4096, 8192):
        T = n // 16
        t, g = layout(n)
        sig = np.isfinite(t) & (t != 0)
        assert sig.sum() == sum(len(r) for r, _ in g.values()) and np.all((t[sig] >= 0.5) & (t[sig] <= 1.0))
        slots = {k: sorted(set((r // T).tolist())) for k, (r, c) in g.items()}
        assert slots["first"] == [0] and slots["tile_end"] == [1, 3] and slots["alone"] == [4, 7] and slots["last"] == [12, 15]
        sr, sc = g["straddle"]
        for cc in set(sc.tolist()):                                               # quarters 1 and 2 in one column, and no other
            assert {8 * T - 1, 8 * T} <= set(sr[sc == cc].tolist()) and set((sr[sc == cc] // (4 * T)).tolist()) == {1, 2}
        cols = {k: sorted(set(c.tolist())) for k, (r, c) in g.items()}
        assert cols["first"] == [0] and cols["tile_end"] == [3] and cols["last"] == [n - 1]
        assert cols["alone"][0] % 4 == 1 and cols["straddle"][0] % 4 == 2 and cols["straddle"][1] == cols["straddle"][0] + 1
        assert len(set(c % 4 for c in cols["lattice"])) == 4 and len(g["lattice"][0]) == (200 if n >= 4096 else 40)
        flagged = (sig | np.isnan(t)).any(axis=0)
        a = cols["alone"][0]
        assert flagged[4 * (a // 4):4 * (a // 4) + 4].sum() == 1                  # alone in its tile
        nan_only = np.isnan(t).any(axis=0) & ~sig.any(axis=0)
        col, r0, r1 = noise_only_column((n, n))
        assert nan_only[col] and flagged[4 * (col // 4):4 * (col // 4) + 4].sum() == 1 and np.isnan(t[:, col]).sum() == r1 - r0
        for k in ("first", "tile_end", "alone", "last"):
            assert not np.isnan(t[:, cols[k]]).any(), k                          # bit 1 without bit 2
        assert np.mean(flagged.reshape(-1, 4).any(axis=1)) < (0.05 if n >= 4096 else 0.5)       # most tiles are empty
        for k, (r, c) in g.items():                                               # spots: 4 rows apart within a column
            for cc in set(c.tolist()):
                d = np.diff(np.sort(r[c == cc]))
                assert np.all((d >= 4) | ((k in ("first", "straddle")) & (d == 1))), (k, cc)    # (rows 0, 1 and 8T-1, 8T: the table's own pairs)


def test_sparse_transform_equals_fft2_at_the_signal_pixels():
    _, _, ref = _oracle_state()
    assert rel_l2(ref["F"], ref["F_full_at_signal"]) < 1e-12


def test_restatement_equals_one_more_oracle_body():
    """Teacher-forced: a float64 oracle from (phase, weights, iter = 2) of the state the restatement started from."""
    o, groups, ref = _oracle_state()
    o3 = orc.OracleHologram(o.target.copy(), phase=o.phase.copy(), slm_shape=o.slm_shape, dtype=np.float64)
    o3.weights, o3.iter = o.weights.copy(), 2
    o3.optimize("WGS-Leonardo", maxiter=1, mraf_factor=MRAF, populate=False)
    assert phase_rel_l2(ref["phase"], o3.phase) < 1e-12 and rel_l2(ref["weights"], o3.weights) < 1e-12
    assert abs(ref["wnorm2"] - (1 + ref["D"])) < 1e-12 and abs(ref["D"] - sum(ref["D_g"].values())) < 1e-12
    # without an update: one GS body from the same state
    g3 = orc.OracleHologram(o.target.copy(), phase=o.phase.copy(), slm_shape=o.slm_shape, dtype=np.float64)
    g3.weights = o.weights.copy()
    g3.optimize("GS", maxiter=1, mraf_factor=MRAF, populate=False)
    plain = reference_body(o.target, groups, o.phase, o.weights, MRAF, EXPONENT, update=False)
    assert phase_rel_l2(plain["phase"], g3.phase) < 1e-12 and plain["D"] == 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _hologram(target, slm, sparse, seed=SEED):
    from slmsuite_amd import _lib as L
    from slmsuite_amd.holography.algorithms import Hologram
    return Hologram(np.array(target, copy=True), phase=synth.seed_phase(seed, slm), slm_shape=slm, dtype=np.float32,
                    engine_options={L.OPT_SPARSE_COLUMNS: sparse})


def _state(h):
    """(phase, weights) downloaded now; each download is an array of its own, and reading changes nothing on the device."""
    return h.phase, h.weights


def _close(h):
    """Destroy the engine without the trailing transform and the downloads of _release_engine (nobody reads them here)."""
    e, h._engine = h._engine, None
    e.close()


def _weights_distance(a, b):
    """rel_l2 of two full weight arrays; equal bytes (what the two forms give: D does not reach the weights) need no
    float64 copies of 16.7 M pixels."""
    return 0.0 if np.array_equal(a, b) else rel_l2(a, b)


def _assert_single_inverse(d, n, nr, listed, bodies=1, phase=None, batch=False, split_bodies=0):
    """The record of `bodies` update bodies on the single-inverse form: which instances ran, and no joining row launch
    but those of the `split_bodies` updates that took the split form (the first update of a run)."""
    fl = (["list"] if listed else []) + (["batch"] if batch else [])
    wo = ([] if listed else ["list"]) + ([] if batch else ["batch"])
    assert d.count("col_presum_kernel") == bodies and d.count("col_tile_kernel", RULE=5) == bodies, d
    assert d.count("col_presum_kernel", N=n, NR=nr, flags=["col_flags"] + (["batch"] if batch else [])) == bodies, d
    kw = {} if phase is None else {"PHASE": phase}
    assert d.count("col_tile_kernel", N=n, NR=nr, RULE=5, EXTRAS=True, flags=fl, without=wo, **kw) == bodies, d
    assert d.count("col_tile_kernel", RULE=5, flags=["col_flags"]) == (bodies if listed else 0), d
    assert d.count("col_tile_kernel", N=n, RULE=3) + d.count("col_tile_kernel", N=n, RULE=4) == split_bodies, d
    assert d.count("row_kernel", N=n, SPLIT=True) == split_bodies and d.count("row_kernel", SPLIT=True) == split_bodies, d


@gpu
def test_combined_layout_one_body_against_float64():
    """
    Every group in one target, 4096 x 4096, SLM 1000 x 1280 (NR = 4), WGS-Leonardo, mraf_factor 0.5, dense launches: the
    third body -- col_presum_kernel + RULE 5, from the engine's own state after two -- against the float64 restatement,
    after the reference has shown that it would notice each group (and the NaN-only column) going missing.

    Measured (MI355X): phase 2.6e-7, weights 6.7e-8 (bounds 5e-6 / 3e-6).  D = 9.97 (||w'||^2 = 10.97: the update
    triples the weights, so 1 / sqrt(1 + D) matters).  Mutants of the reference, distance from its phase: first 6.2e-3,
    tile_end 5.2e-3, alone 6.1e-3, straddle 1.9e-3, last 4.2e-3, lattice 0.17, NaN-only column 1.8e-4 (needed: 5e-5).
    Conditioning |F| / (||F|| T sqrt(S / P)): 0.30 .. 1.85 (without the factor: 0.084 .. 0.51).  With the odd half of
    the ``sig_rows`` word read as the even one (a build made for this purpose) the test fails: see DESIGN.md, section 5.
    """
    slm = SLMS[0]
    target, groups = layout(4096)
    h = _hologram(target, slm, 0)
    h.optimize("WGS-Leonardo", maxiter=2, verbose=False, mraf_factor=MRAF)
    p2, w2 = _state(h)                         # (reading does not clear "the stored weights are normalised")
    dispatch_of(h)
    h.optimize("WGS-Leonardo", maxiter=1, verbose=False, mraf_factor=MRAF)
    _assert_single_inverse(dispatch_of(h), 4096, 4, listed=False, phase=0)
    ref = reference_body(h.target, groups, p2, w2, MRAF, EXPONENT)
    assert_conditioned(ref)
    dist = assert_sensitive(ref, groups)
    p3, w3 = _state(h)
    _close(h)
    assert np.all(np.isfinite(p3)) and np.all(np.isfinite(w3))
    ep, ew = phase_rel_l2(p3, ref["phase"]), weights_rel_l2(w3, ref)
    report("MRAF layouts: combined, body 3 vs float64", phase=ep, weights=ew, nearest_mutant=min(dist.values()), D=ref["D"],
           ratio_min=ref["ratio"].min(), ratio_max=ref["ratio"].max())
    print("combined layout vs float64: phase", ep, "weights", ew, "mutants", dist)
    assert ep < PHASE_BOUND and ew < WEIGHT_BOUND, (ep, ew)


AB_CASES = [pytest.param(4096, SLMS[i % 3], (g,), "WGS-Leonardo", {}, 0, id=f"{g}-nr{4 + i % 3}") for i, g in enumerate(GROUPS)] + [
    pytest.param(4096, SLMS[0], GROUPS, "WGS-Leonardo", {}, 0, id="combined-nr4"),
    pytest.param(4096, SLMS[1], GROUPS, "WGS-Kim", dict(fix_phase_iteration=2), 0, id="combined-kim"),     # PHASE 1, then PHASE 2
    pytest.param(4096, SLMS[2], GROUPS, "WGS-Leonardo", {}, 1, id="combined-engine-default"),              # the tile list
    pytest.param(8192, (1152, 1920), GROUPS, "WGS-Leonardo", {}, 0, id="combined-8192"),                   # T = 512
]


@gpu
@pytest.mark.parametrize("n, slm, names, method, extra, sparse", AB_CASES)
def test_single_inverse_matches_the_split_form(n, slm, names, method, extra, sparse, monkeypatch):
    """
    Three bodies with the single-inverse form on the third (HGS_MRAF_PRESUM=1) against the split form on every update
    (=0), bounds of test_mraf_single_inverse_matches_the_split_form: weights 1e-6, phase 3e-6 and > 0.  Each group on its
    own with the noise box (SLM cycled, so 4, 5 and 6 slots each meet an edge layout), all together, WGS-Kim fixing the
    phase in body 2, the engine's default (tile list), and 8192 x 8192 -- there also the weights of body 3 against the
    sparse float64 restatement (3e-6; no full transform needed).

    Measured (MI355X): weights identical in all ten cases (0.0: D does not reach them); phase 8.5e-8 (straddle) ..
    2.0e-7 (combined), WGS-Kim 1.8e-7, engine default 1.8e-7, 8192 x 8192 1.3e-7; there weights vs float64 8.7e-8.
    """
    target, groups = layout(n, tuple(names))
    nr = tile_slots((n, n), slm)
    out = {}
    for presum in ("1", "0"):
        monkeypatch.setenv("HGS_MRAF_PRESUM", presum)
        h = _hologram(target, slm, sparse)
        h.optimize(method, maxiter=2, verbose=False, mraf_factor=MRAF, **extra)
        two = _state(h) if (n == 8192 and presum == "1") else None       # (what the float64 restatement starts from)
        d = dispatch_of(h)
        split = d.count("col_tile_kernel", N=n, RULE=3) + d.count("col_tile_kernel", N=n, RULE=4)
        assert split == 1 and d.count("row_kernel", SPLIT=True) == 1 and d.count("col_presum_kernel") == 0, d      # body 2
        h.optimize(method, maxiter=1, verbose=False, mraf_factor=MRAF, **extra)
        d = dispatch_of(h)
        if presum == "1":
            _assert_single_inverse(d, n, nr, listed=bool(sparse), phase=2 if "Kim" in method else 0)
        else:
            assert d.count("col_presum_kernel") == 0 and d.count("col_tile_kernel", RULE=5) == 0, d
            split = d.count("col_tile_kernel", N=n, RULE=3) + d.count("col_tile_kernel", N=n, RULE=4)
            assert split == 1 and d.count("row_kernel", SPLIT=True) == 1, d
        out[presum] = _state(h)
        if two is not None:
            ref = reference_body(h.target, groups, two[0], two[1], MRAF, EXPONENT, full=False)
        _close(h)
    ep, ew = phase_rel_l2(out["1"][0], out["0"][0]), _weights_distance(out["1"][1], out["0"][1])
    errs = dict(phase=ep, weights=ew)
    if n == 8192:
        errs["weights_vs_float64"] = weights_rel_l2(out["1"][1], ref)
    report(f"MRAF layouts: single-inverse vs split, {n} {slm} {method} {'+'.join(names)} sparse={sparse}", **errs)
    print("single-inverse vs split", n, slm, method, names, errs)
    assert np.all(np.isfinite(out["1"][0])) and np.all(np.isfinite(out["1"][1]))
    assert ew < 1e-6 and ep < 3e-6 and ep > 0, errs
    if n == 8192:
        assert errs["weights_vs_float64"] < WEIGHT_BOUND, errs


@gpu
def test_rule_6_one_gs_body_against_float64():
    """
    MRAF without a weight update (col_tile_kernel RULE 6): one GS body from the seed on the combined layout, dense and
    over the tile list (the engine's default; only there do the scan's column flags go with the launch, and the inverse of
    a column is skipped where its flags have neither bit 1 nor bit 2), against the restatement with w' = w.  A column
    wrongly taken for empty loses its whole part: the reference without the NaN-only column lies ten bounds away.

    Measured (MI355X): phase 1.4e-6 (bound 5e-6), the same bytes with and without the list; ``col_flags`` went with the
    listed launch and not with the dense one.
    """
    slm = SLMS[1]
    target, groups = layout(4096)
    nr = tile_slots((4096, 4096), slm)
    ref = None
    for sparse in (0, 1):
        h = _hologram(target, slm, sparse)
        p0, w0 = h.phase.copy(), np.nan_to_num(h.target, nan=0.0)            # reset weights: the target with NaN -> 0
        h.optimize("GS", maxiter=1, verbose=False, mraf_factor=MRAF)
        d = dispatch_of(h)
        fl, wo = (["list"], []) if sparse else ([], ["list"])
        assert d.count("col_tile_kernel") == 1 and d.count("col_presum_kernel") == 0, d
        assert d.count("col_tile_kernel", N=4096, NR=nr, RULE=6, EXTRAS=True, PHASE=0, flags=fl, without=wo + ["batch"]) == 1, d
        carried = d.count("col_tile_kernel", RULE=6, flags=["col_flags"])
        assert carried == sparse, d                                         # the flags travel with the list, not without
        if ref is None:
            ref = reference_body(h.target, groups, p0, w0, MRAF, EXPONENT, update=False)
            assert phase_rel_l2(ref["mutants"]["noise_only"], ref["phase"]) >= 10 * PHASE_BOUND
        p1 = h.phase
        _close(h)
        ep = phase_rel_l2(p1, ref["phase"])
        report(f"MRAF layouts: RULE 6, one GS body vs float64, sparse={sparse}", phase=ep, col_flags=carried)
        print("RULE 6 vs float64: sparse", sparse, "col_flags", carried, "phase", ep)
        assert np.all(np.isfinite(p1)) and ep < PHASE_BOUND, (sparse, ep)


@gpu
def test_batch_of_two_with_different_layouts():
    """
    Scan flags and ``sig_rows`` are indexed per hologram: hologram 0 holds ``first``, ``alone`` and ``last``, hologram 1
    ``tile_end``, ``straddle`` and a NaN-only column (in a tile that is empty in hologram 0).  Three bodies, the third on
    col_presum_kernel + RULE 5 with grid.y = 2; each hologram against an engine of its own within the 5e-6 of
    test_batch_matches_single (phase and weights).  Measured (MI355X): 0.0 and 0.0 for both holograms (the same bytes).
    """
    from slmsuite_amd import _lib as L
    from slmsuite_amd.batch import HologramBatch
    from slmsuite_amd.holography.algorithms import Hologram
    n, slm = 4096, SLMS[0]
    targets = [layout(n, ("first", "alone", "last"), False)[0], layout(n, ("tile_end", "straddle"), n // 8 + 3)[0]]
    phases = np.stack([synth.seed_phase(60 + b, slm) for b in range(2)])
    hb = HologramBatch((n, n), slm, np.stack(targets), phases)
    hb.optimize("WGS-Leonardo", 3, mraf_factor=MRAF)
    d = dispatch_of(hb)
    _assert_single_inverse(d, n, tile_slots((n, n), slm), listed=True, batch=True, split_bodies=1)       # body 2 split, body 3 single
    pb, wb = hb.phases(), hb.engine.get(L.WEIGHTS)
    hb.close()
    for b in range(2):
        h = Hologram(np.array(targets[b], copy=True), phase=phases[b].copy(), slm_shape=slm, dtype=np.float32)
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False, mraf_factor=MRAF)
        _assert_single_inverse(dispatch_of(h), n, tile_slots((n, n), slm), listed=True, split_bodies=1)
        ep, ew = phase_rel_l2(pb[b], h.phase), _weights_distance(wb[b], h.weights)
        _close(h)
        report(f"MRAF layouts: batch of two, hologram {b} vs a single engine", phase=ep, weights=ew)
        print("batch vs single: hologram", b, "phase", ep, "weights", ew)
        assert np.all(np.isfinite(pb[b])) and np.all(np.isfinite(wb[b]))
        assert ep < 5e-6 and ew < 5e-6, (b, ep, ew)
