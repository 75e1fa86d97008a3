"""
The two complex GEMMs of CompressedSpotHologram's separable path (cgemm_streamk<1>: nearfield -> farfield with the y
contraction in its epilogue, cgemm_streamk<0>: farfield -> nearfield) under every regime of their stream-K schedule,
operator by operator against float64 direct (non-separable) summation over every spot and every pixel.

The schedule cuts the tiles x KT k-steps of a GEMM into G = min(2 #CU, tiles KT) shares.  At the sizes the other
separable tests use that is one step per workgroup: no prefetch, no tile boundary inside a range, no whole tile in a
range.  HGS_OPT_SEP_WORKGROUPS caps G, which brings every regime to a 150 x 200 SLM (what each cap reaches is asserted on
the schedule itself in tests/test_streamk_schedule.py):

  cap 1   one workgroup walks all 6 (f2n: 4) tiles, every tile whole;
  cap 2   ranges of 3 and 2 whole tiles;
  cap 3   n2f: 26 steps = exactly two tiles, ranges end ON a boundary; f2n: a crossing and a whole tile in one range;
  cap 5   crossings and whole tiles, 2 planes;     cap 7   crossings without a whole tile, 2 - 3 planes;
  cap 16  several workgroups per tile, multi-step ranges (the prefetch runs), 4 planes;
  cap 0   one step per workgroup, 13 and 19 planes (on 256 CUs).

Errors are measured per OUTPUT TILE -- rel_l2 over each block of 128 spots, phase_rel_l2 over each 128 x 128 block of the
SLM -- so that a defect confined to one tile is not diluted.  Bounds: what tests/test_full_configs.py holds for this path
at full size (2e-5 on the farfield, 1e-4 on the phase phasor; measured there 2e-6 .. 4e-6 at K = 1920 and 1e4), applied
to every tile: smaller K only rounds less, and a lost or misplaced k-step is at least 1 / KT ~ 5e-2 of a tile.
"""
import numpy as np
import pytest

from conftest import dispatch_of, rel_l2, phase_rel_l2, report
from slmsuite_amd import _lib as L
from slmsuite_amd import synth
from slmsuite_amd.engine import Engine, make_step
from slmsuite_amd.hardware import SimpleFourierSLM, SimpleSLM
from slmsuite_amd.holography import toolbox
from slmsuite_amd.holography.algorithms import CompressedSpotHologram

pytestmark = pytest.mark.gpu

TOL_FF, TOL_PH = 2e-5, 1e-4
SMALL, SMALL_N, SMALL_CAPS = (150, 200), 300, (1, 2, 3, 5, 7, 16, 0)
EXACT, EXACT_N, EXACT_CAPS = (128, 256), 256, (1, 3, 0)


class _GaussianSLM(SimpleSLM):
    """An SLM whose source amplitude is an array that varies over the aperture."""

    def _get_source_amplitude(self):
        h, w = self.shape
        y, x = np.mgrid[0:h, 0:w]
        return np.exp(-(((x - 0.45 * w) / (0.6 * w)) ** 2 + ((y - 0.55 * h) / (0.7 * h)) ** 2))


class _Problem:
    """One (SLM shape, spot count, D): inputs, and the float64 kernel phasors every cap is checked against (made once)."""

    def __init__(self, slm_shape, N, D, seed, direct=True):
        from oracle import hgs_oracle as orc
        self.slm_shape, self.N, self.D = slm_shape, N, D
        self.fs = SimpleFourierSLM(_GaussianSLM(slm_shape, pitch_um=(8, 8), wav_um=0.78))
        v = np.vstack([0.03 * (synth.uniform01(seed, (N,), k) - 0.5) for k in range(2)])
        if D == 3:
            v = np.vstack((v, 4e-6 * (synth.uniform01(seed, (N,), 2) - 0.5)))
        self.v = v
        self.spot_amp = 0.5 + synth.uniform01(seed + 1, (N,), 0)
        self.kern = (0.3 * synth.seed_phase(seed + 2, slm_shape)).astype(np.float32)
        self.phase0 = synth.seed_phase(seed + 3, slm_shape)
        h = self.hologram(0)
        self.terms, self.wts = orc.monomial_weights(h.zernike_basis, h.spot_zernike)
        self.xg = np.asarray(h._xg, dtype=np.float64)
        self.yg = np.asarray(h._yg, dtype=np.float64)
        self.amp_nf = np.asarray(h.amp, dtype=np.float64).ravel()
        assert self.amp_nf.size == slm_shape[0] * slm_shape[1] and np.ptp(self.amp_nf) > 0.1 * self.amp_nf.max()
        # E[n, p] = exp(i phi_n(p)), float64, every spot and pixel (as tests/test_compressed.py::_kernel_phase64)
        self.E = np.exp(1j * self.kernel_phase(np.arange(N), np.arange(self.amp_nf.size))) if direct else None

    def hologram(self, cap):
        h = CompressedSpotHologram(self.v, basis="kxy", spot_amp=self.spot_amp, cameraslm=self.fs, propagation_kernel=self.kern,
                                   engine_options={L.OPT_SEPARABLE: 1, L.OPT_SEP_WORKGROUPS: cap})
        h.reset_phase(self.phase0)
        return h

    def kernel_phase(self, spots, pix):
        x, y = self.xg.ravel()[pix], self.yg.ravel()[pix]
        phi = np.zeros((len(spots), len(pix)))
        for m, (px, py) in enumerate(self.terms):
            assert px >= 0 and py >= 0
            phi += self.wts[m, spots][:, None] * (x ** int(px) * y ** int(py))[None, :]
        return phi

    def nearfield(self, phase):
        return self.amp_nf * np.exp(1j * (np.asarray(phase, dtype=np.float64).ravel() + self.kern.astype(np.float64).ravel()))

    # direct float64 summation
    def ref_farfield(self, phase):
        ref = np.conj(self.E) @ self.nearfield(phase)
        return ref / np.sqrt(np.sum(np.abs(ref) ** 2))

    def ref_phase(self, ffc):
        nf = np.asarray(ffc, dtype=np.complex128) @ self.E
        return (np.angle(nf) - self.kern.astype(np.float64).ravel()).reshape(self.slm_shape)


def _ff_tiles(ff, ref):
    """rel_l2 per block of 128 spots (the row tiles of the n2f GEMM)."""
    return [rel_l2(ff[i:i + 128], ref[i:i + 128]) for i in range(0, len(ref), 128)]


def _phase_tiles(ph, ref):
    """phase_rel_l2 per 128 x 128 block of the SLM (the output tiles of the f2n GEMM)."""
    H, W = ref.shape
    ph = np.asarray(ph).reshape(H, W)
    return [phase_rel_l2(ph[y:y + 128, x:x + 128], ref[y:y + 128, x:x + 128]) for y in range(0, H, 128) for x in range(0, W, 128)]


def _n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _assert_dispatch(d, capped):
    assert d.families() == {"cgemm_streamk"}, d
    assert d.count("cgemm_streamk", EPI=1) > 0 and d.count("cgemm_streamk", EPI=0) > 0, d
    if capped:
        assert d.count("cgemm_streamk", without=("sk_cap",)) == 0, d
    else:
        assert d.count("cgemm_streamk", flags=("sk_cap",)) == 0, d


def _one_body(prob, h, e, weights):
    """nearfield2farfield, farfield_constraint, farfield2nearfield on phase0 and the given weights: (ff, ffc, phase) of the
    engine.  Every run that is compared with another starts from the same weights: what differs is the schedule alone."""
    e.set(L.PHASE, prob.phase0)
    e.set(L.WEIGHTS, weights)
    e.nearfield2farfield()
    ff = e.get(L.FARFIELD)[0].astype(np.complex128)
    e.farfield_constraint(h._make_step())
    ffc = e.get(L.FARFIELD)[0].astype(np.complex128)
    e.farfield2nearfield()
    ph = e.get(L.PHASE)[0].copy()
    return ff, ffc, ph


def _run_caps(prob, caps, label, steps):
    """Every cap on one problem: per-tile float64 bounds, the dispatch flag, agreement between any two caps."""
    ref_ff = prob.ref_farfield(prob.phase0)
    out, w0 = {}, None
    for cap in caps:
        h = prob.hologram(cap)
        h.optimize("WGS-Leonardo", maxiter=2, verbose=False)          # (the fused loop under this cap)
        if w0 is None:
            w0 = np.array(h.weights, copy=True)                       # weights away from the target, the same for every cap
        capped = 0 < cap < min(2 * _n_cu(), min(steps))
        assert cap == 0 or capped, "the shapes of this file have more steps than any cap"
        _assert_dispatch(dispatch_of(h), capped)
        e = h._get_engine()
        ff, ffc, ph = _one_body(prob, h, e, w0)
        _assert_dispatch(dispatch_of(h), capped)
        t_ff, t_ph = _ff_tiles(ff, ref_ff), _phase_tiles(ph, prob.ref_phase(ffc))
        report(f"stream-K {label} D={prob.D} cap {cap} vs float64 direct summation, worst tile",
               farfield=max(t_ff), phase=max(t_ph), farfield_all=rel_l2(ff, ref_ff))
        assert max(t_ff) < TOL_FF, (cap, t_ff)
        assert max(t_ph) < TOL_PH, (cap, t_ph)
        out[cap] = (ff, ph)
        h._release_engine()
    worst_ff = worst_ph = 0.0
    for i, a in enumerate(caps):
        for b in caps[i + 1:]:
            worst_ff = max(worst_ff, max(_ff_tiles(out[a][0], out[b][0])))
            worst_ph = max(worst_ph, max(_phase_tiles(out[a][1], out[b][1].astype(np.float64))))
    report(f"stream-K {label} D={prob.D} any two caps, worst tile", farfield=worst_ff, phase=worst_ph)
    assert worst_ff < TOL_FF and worst_ph < TOL_PH
    # the knob reached the launch: one workgroup and one workgroup per step group the fp32 partial sums differently
    assert not np.array_equal(out[1][0], out[0][0]) and not np.array_equal(out[1][1], out[0][1])
    return out


_PROBLEMS = {}


def _problem(slm_shape, N, D, seed):
    """The small problems are shared between the tests of this file: their float64 phasors are tabulated once."""
    key = (slm_shape, N, D)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = _Problem(slm_shape, N, D, seed)
    return _PROBLEMS[key]


@pytest.mark.parametrize("D", [2, 3])
def test_small_shape_every_cap_against_float64_sums(D):
    """
    SLM (150, 200), 300 spots of varying amplitude, an array source amplitude and a propagation kernel.  n2f: 3 x 2 tiles,
    KT = 13 (the last spot tile holds 44 rows, the last H tile 22, the last k-step is half padding); f2n: 2 x 2 tiles,
    KT = 19.  Caps {1, 2, 3, 5, 7, 16, 0}: the regimes of this file's docstring.
    """
    _run_caps(_problem(SMALL, SMALL_N, D, 81), SMALL_CAPS, "small (150, 200) N=300", steps=(3 * 2 * 13, 2 * 2 * 19))


@pytest.mark.parametrize("D", [2, 3])
def test_exact_multiple_shape_against_float64_sums(D):
    """SLM (128, 256), 256 spots: every m < M / n < N guard is trivially true and no operand is padded."""
    _run_caps(_Problem(EXACT, EXACT_N, D, 91), EXACT_CAPS, "exact (128, 256) N=256", steps=(2 * 1 * 16, 1 * 2 * 16))


def test_cap_set_after_the_tables_exist_rebuilds_them():
    """
    HGS_OPT_SEP_WORKGROUPS on an engine whose kernels are uploaded: the schedule tables and the two plane buffers they
    size (sk_tab, sep_c1, sep_c2) are rebuilt.  0 -> 3 (19 planes -> 2) -> 0: the capped run meets the float64 bounds and
    equals an engine that was created capped bit for bit; back at 0 the first results return bit for bit (a buffer still
    sized for 2 planes would be written 17 planes past its end).  Negative values are an argument error.
    """
    prob = _problem(SMALL, SMALL_N, 2, 81)
    ref_ff = prob.ref_farfield(prob.phase0)
    h = prob.hologram(0)
    h.optimize("WGS-Leonardo", maxiter=2, verbose=False)
    w0 = np.array(h.weights, copy=True)
    e = h._get_engine()
    dispatch_of(h)

    def body():
        return _one_body(prob, h, e, w0)

    first = body()
    _assert_dispatch(dispatch_of(h), False)
    with pytest.raises(ValueError):
        e.set_option(L.OPT_SEP_WORKGROUPS, -1)
    e.set_option(L.OPT_SEP_WORKGROUPS, 3)
    capped = body()
    _assert_dispatch(dispatch_of(h), True)
    t_ff, t_ph = _ff_tiles(capped[0], ref_ff), _phase_tiles(capped[2], prob.ref_phase(capped[1]))
    report("stream-K small D=2 cap 3 set after the tables, worst tile", farfield=max(t_ff), phase=max(t_ph))
    assert max(t_ff) < TOL_FF and max(t_ph) < TOL_PH
    assert not np.array_equal(capped[0], first[0])
    e.set_option(L.OPT_SEP_WORKGROUPS, 0)
    again = body()
    _assert_dispatch(dispatch_of(h), False)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    h._release_engine()
    # an engine created with the cap
    h3 = prob.hologram(3)
    h3.optimize("WGS-Leonardo", maxiter=2, verbose=False)
    born = _one_body(prob, h3, h3._get_engine(), w0)
    for a, b in zip(capped, born):
        np.testing.assert_array_equal(a, b)
    h3._release_engine()


def test_natural_schedule_beyond_one_step_per_workgroup():
    """
    No cap: SLM (768, 1024), 400 spots, D = 3.  On 256 CUs n2f has 4 x 6 tiles of 64 k-steps (1536 steps, 3.0 per
    workgroup, 22 planes) and f2n 6 x 8 tiles of 25 (1200 steps, 2.34 per workgroup, 11 planes); 16 workgroups of each
    cross a tile boundary.  Direct summation of 400 x 786 k terms is too slow for a test: the reference is the float64
    SEPARABLE product (Ex, Ey tabulated in float64, contracted with numpy.matmul), itself held to 1e-12 of direct float64
    summation on 16 spots x all pixels and on 512 pixels x all spots.
    """
    n_cu = _n_cu()
    if n_cu != 256:
        print(f"skipped: the device reports {n_cu} CUs, the premise of this test is the schedule on 256")
        pytest.skip(f"the device reports {n_cu} CUs; this test pins the schedule 256 CUs give")
    shape, N = (768, 1024), 400
    H, W = shape
    steps = (4 * 6 * 64, 6 * 8 * 25)
    assert all(s > 2 * (2 * n_cu) for s in steps)               # more than two steps per workgroup
    prob = _Problem(shape, N, 3, 101, direct=False)
    assert np.all(prob.xg == prob.xg[0][None, :]) and np.all(prob.yg == prob.yg[:, 0][:, None])      # a product grid
    xs, ys = prob.xg[0], prob.yg[:, 0]
    fx, fy = np.zeros((N, W)), np.zeros((N, H))
    for m, (px, py) in enumerate(prob.terms):
        assert px >= 0 and py >= 0 and (px == 0 or py == 0)
        if py == 0:
            fx += prob.wts[m][:, None] * (xs ** int(px))[None, :]
        else:
            fy += prob.wts[m][:, None] * (ys ** int(py))[None, :]
    Ex, Ey = np.exp(1j * fx), np.exp(1j * fy)                   # exp(i phi_n(x, y)) = Ex[n, x] Ey[n, y]

    h = prob.hologram(0)
    h.optimize("WGS-Leonardo", maxiter=2, verbose=False)
    _assert_dispatch(dispatch_of(h), False)
    ff, ffc, ph = _one_body(prob, h, h._get_engine(), np.array(h.weights, copy=True))
    _assert_dispatch(dispatch_of(h), False)
    h._release_engine()

    nf = prob.nearfield(prob.phase0).reshape(H, W)
    raw = np.sum(np.conj(Ey) * np.matmul(np.conj(Ex), nf.T), axis=1)            # sum_y Ey* (sum_x Ex* nf)
    ref_ff = raw / np.sqrt(np.sum(np.abs(raw) ** 2))
    nfb = np.matmul((Ey * ffc[:, None]).T, Ex)                                  # sum_n ffc_n Ey[n, y] Ex[n, x]
    ref_ph = np.angle(nfb) - prob.kern.astype(np.float64)
    # the separable reference against direct summation
    rng = np.random.default_rng(102)
    spots = np.sort(rng.choice(N, 16, replace=False))
    pix = np.sort(rng.choice(H * W, 512, replace=False))
    direct_ff = np.exp(-1j * prob.kernel_phase(spots, np.arange(H * W))) @ nf.ravel()
    direct_nf = ffc @ np.exp(1j * prob.kernel_phase(np.arange(N), pix))
    sep_err = dict(farfield=rel_l2(raw[spots], direct_ff), nearfield=rel_l2(nfb.ravel()[pix], direct_nf))
    t_ff, t_ph = _ff_tiles(ff, ref_ff), _phase_tiles(ph, ref_ph)
    report("stream-K natural schedule (768, 1024) N=400 D=3 vs float64, worst tile", farfield=max(t_ff), phase=max(t_ph),
           separable_ref_farfield=sep_err["farfield"], separable_ref_nearfield=sep_err["nearfield"])
    assert sep_err["farfield"] < 1e-12 and sep_err["nearfield"] < 1e-12, sep_err
    assert max(t_ff) < TOL_FF, t_ff
    assert max(t_ph) < TOL_PH, t_ph


@pytest.mark.parametrize("cap", [3, 0])
def test_batch_of_two_equals_single_runs(cap):
    """
    A raw kind-1 engine with batch = 2 on the small shape, two different phases: the per-batch operand strides (n2f: A
    shared, B per hologram; f2n the reverse) and the b * planes + seg plane indexing.  Each hologram equals its batch-1
    run bit for bit and meets the float64 bounds.
    """
    prob = _problem(SMALL, SMALL_N, 3, 81)
    h = prob.hologram(cap)                                   # host-side set-up only: grids, kernels, target, amplitude
    terms, w = toolbox.zernike_monomial_weights(h.zernike_basis, h.spot_zernike)
    phases = np.stack([prob.phase0, synth.seed_phase(85, SMALL)]).astype(np.float32)
    step = make_step(dict(method="WGS-Leonardo", feedback="computational"), 0, spot_window=1)

    def run(batch, phase):
        e = Engine(SMALL, SMALL, np.float32, batch=batch, n_spots=SMALL_N, kind=1, n_monomials=terms.shape[0])
        e.set_option(L.OPT_SEPARABLE, 1)
        e.set_option(L.OPT_SEP_WORKGROUPS, cap)
        e.set(L.AMP, h.amp)
        e.set(L.PROP_KERNEL, prob.kern)
        e.set(L.XGRID, h._xg)
        e.set(L.YGRID, h._yg)
        e.set(L.TARGET, h.target)
        e.set(L.MONOMIALS, terms)
        e.set(L.SPOT_COEFF, w)
        e.reset_weights()
        e.set(L.PHASE, phase)
        e.nearfield2farfield()
        ff = e.get(L.FARFIELD).copy()
        e.farfield_constraint(step)
        ffc = e.get(L.FARFIELD).copy()
        e.farfield2nearfield()
        ph = e.get(L.PHASE).copy()
        d = dispatch_of(e)
        _assert_dispatch(d, cap > 0)
        assert d.count("cgemm_streamk", flags=("batch",)) == (2 if batch > 1 else 0), d
        e.close()
        return ff, ffc, ph

    both = run(2, phases)
    worst = dict(farfield=0.0, phase=0.0)
    for b in range(2):
        one = run(1, phases[b])
        for got, want in zip(both, one):
            np.testing.assert_array_equal(got[b], want[0])
        t_ff = _ff_tiles(both[0][b].astype(np.complex128), prob.ref_farfield(phases[b]))
        t_ph = _phase_tiles(both[2][b], prob.ref_phase(both[1][b]))
        worst = dict(farfield=max(worst["farfield"], max(t_ff)), phase=max(worst["phase"], max(t_ph)))
        assert max(t_ff) < TOL_FF and max(t_ph) < TOL_PH, (b, t_ff, t_ph)
    report(f"stream-K batch of two, small shape D=3 cap {cap}, worst tile", **worst)
    assert not np.array_equal(both[2][0], both[2][1])
