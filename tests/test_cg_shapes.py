"""
optimize(method="CG") at the shapes, settings and engine states the fixtures of tests/test_cg.py do not reach: element counts
that are no multiple of four (the tail lanes of cg_seed_kernel / cg_adam_kernel), rows of 512 .. 4096 points with the complex
nearfield output of f2n_complex (both forms of row_kernel, the shifted eight-slot one included), a padded image large
enough for a second trip of the seed pass's grid-stride loop, other Adam settings than the defaults, exact zeros in the
farfield, and the hand-overs between GS, hgs_reset and hgs_cg_iterate.

The high-precision reference of every GPU test is the float64 NumPy restatement of one loop body kept in tests/test_cg.py
(np_loss_and_gradient + adam_step), which test_numpy_restatement_reproduces_reference ties to the reference project below
1e-10 at the default settings and test_restatement_matches_torch_adam (here) to torch's autograd and Adam at two others.
The engine and the restatement get the same inputs: what the hologram holds after its own normalisation, as float64.

Two error measures: relative L2, and the largest absolute error over the RMS of the reference (one bad pixel among S moves
the second by about 1, the first by about 1 / sqrt(S) >= 2e-2 at the sizes here).  Bounds:

* float64: both <= 1e-9 (the project's fp64 discriminator), the loss relative 1e-12.
* float32, power-of-two padded shapes: 3 * d32, d32 = the same measure between a float32 CPU evaluation of the same body
  (torch.fft in complex64, the restatement's formula) and the float64 restatement, per geometry; the loss within 3 * d32 of the
  gradient's relative L2 as in test_cg.py (the large case: within 3 * its own d32_loss).
* float32, general (Bluestein) lengths: max(3 * d32, 1e-5), 1e-5 being the per-body amp_ff tolerance test_gpu_sweep.py accepts
  on these transforms.

Float32 phases after a step are not compared (module docstring of test_cg.py); that every pixel moved is.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import dispatch_of, load_golden, rel_l2
from slmsuite_amd import _lib as L
from slmsuite_amd.holography import toolbox
from slmsuite_amd.holography.algorithms import Hologram
from test_cg import BETA1, BETA2, EPS, LR, adam_step, make_hologram, np_loss_and_gradient

# (padded shape, SLM shape): P % 4, S % 4 and the transform are asserted by test_residues
TAILS = (((64, 128), (31, 35)), ((64, 128), (30, 35)), ((64, 64), (33, 47)),
         ((65, 65), (32, 48)), ((66, 65), (33, 51)), ((101, 75), (33, 51)))
# row width -> odd SLM width below half of it (trailing transforms, negative leading columns)
ROW_WIDTHS = {512: 201, 1024: 333, 2048: 777, 4096: 1111}
ROWS = tuple(((64, w), slm) for w, odd in ROW_WIDTHS.items() for slm in ((40, w), (33, odd)))
BIG = ((2048, 2048), (1152, 1920))
RESIDUES = {                                     # (P % 4, S % 4)
    ((64, 128), (31, 35)): (0, 1), ((64, 128), (30, 35)): (0, 2), ((64, 64), (33, 47)): (0, 3),
    ((65, 65), (32, 48)): (1, 0), ((66, 65), (33, 51)): (2, 3), ((101, 75), (33, 51)): (3, 3),
    ((64, 512), (40, 512)): (0, 0), ((64, 512), (33, 201)): (0, 1), ((64, 1024), (40, 1024)): (0, 0),
    ((64, 1024), (33, 333)): (0, 1), ((64, 2048), (40, 2048)): (0, 0), ((64, 2048), (33, 777)): (0, 1),
    ((64, 4096), (40, 4096)): (0, 0), ((64, 4096), (33, 1111)): (0, 3), BIG: (0, 0),
}
HYPER = (dict(lr=0.02, betas=(0.8, 0.99), eps=1e-6), dict(lr=0.1, betas=(0.0, 0.5), eps=1e-3))
DTYPES = (np.float64, np.float32)
# "Every pixel moved": asserted where |g| > 10 eps and, beyond that, down to eps / 100.  Gradients of single pixels are small
# (median 3e-8 .. 1e-7 at the tail geometries: 10 eps would look at one pixel in ten), and Adam's first step is
# lr |g| / (|g| + eps) >= lr / 101 = 1e-3 there: four thousand float32 ulps of the largest phase, with the engine's own float32
# gradient error (d32 * RMS, some 1e-14) far below the threshold.
MOVES_ABOVE = 1e-2 * EPS


def is_pow2(shape):
    return all(v & (v - 1) == 0 for v in shape)


# ---- inputs, references, measures ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_inputs(shape, slm, arrays):
    """Target, start phase and -- ``arrays`` -- source amplitude and propagation kernel, as float32-representable float64
    values (both element types start from the same numbers).  Not to be modified: shared between tests."""
    rng = np.random.default_rng([shape[0], shape[1], slm[0], slm[1], int(arrays)])

    def f32(a):
        a = a.astype(np.float32).astype(np.float64)
        a.setflags(write=False)
        return a
    return dict(target=f32(rng.random(shape) ** 3), phase=f32(rng.uniform(-np.pi, np.pi, slm)),
                amp=f32(0.5 + rng.random(slm)) if arrays else None, kernel=f32(rng.uniform(-1, 1, slm)) if arrays else None)


def hologram_of(shape, slm, arrays, dtype, phase=None):
    i, dt = make_inputs(shape, slm, arrays), np.dtype(dtype).type
    return Hologram(i["target"].astype(dt), amp=None if i["amp"] is None else i["amp"].astype(dt),
                    phase=(i["phase"] if phase is None else phase).astype(dt), slm_shape=slm, dtype=dt,
                    propagation_kernel=None if i["kernel"] is None else i["kernel"].astype(dt))


def held_inputs(h):
    """(amp, kernel, target) as the hologram holds them -- normalised in its own element type -- in float64; a scalar
    amplitude as the engine's element type rounds it."""
    dt = np.dtype(h.dtype).type
    amp = float(dt(h.amp)) if np.isscalar(h.amp) else np.array(h.amp, dtype=np.float64)
    kern = None if h.propagation_kernel is None else np.array(h.propagation_kernel, dtype=np.float64)
    return amp, kern, np.array(h.target, dtype=np.float64)


def np_trajectory(phase, amp, kernel, target, steps, lr=LR, betas=(BETA1, BETA2), eps=EPS):
    """``steps`` bodies of the float64 restatement: (first gradient, [phase after each step], losses)."""
    phase = np.array(phase, dtype=np.float64)
    m, v = np.zeros_like(phase), np.zeros_like(phase)
    grad1, phases, losses = None, [], []
    for t in range(1, steps + 1):
        loss, g = np_loss_and_gradient(phase, amp, kernel, target)
        grad1 = g if t == 1 else grad1
        phase, m, v = adam_step(phase, m, v, g, t, lr=lr, betas=betas, eps=eps)
        losses.append(loss)
        phases.append(phase.copy())
    return grad1, phases, np.array(losses)


def f32_loss_and_gradient(phase, amp, kernel, target):
    """np_loss_and_gradient, every operation in float32 / complex64 on the CPU (torch.fft): the yardstick d32."""
    def t32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    shape, slm = target.shape, phase.shape
    i0, i1, i2, i3 = toolbox.unpad(shape, slm)
    arg = t32(phase) if kernel is None else t32(phase) + t32(kernel)
    a = torch.full(slm, float(amp), dtype=torch.float32) if np.isscalar(amp) else t32(amp)
    win = torch.polar(a, arg)
    n = torch.zeros(shape, dtype=torch.complex64)
    n[i0:i1, i2:i3] = win
    F = torch.fft.fftshift(torch.fft.fft2(torch.fft.fftshift(n), norm="ortho"))
    A = F.abs()
    s, M = torch.sqrt(torch.sum(A * A)), F.numel()
    r = A / s - t32(target)
    G = torch.where(A > 0, (2 / (M * s)) * r * F / A, torch.zeros((), dtype=torch.complex64))
    g = torch.fft.ifftshift(torch.fft.ifft2(torch.fft.ifftshift(G), norm="ortho"))[i0:i1, i2:i3]
    assert F.dtype == torch.complex64 and g.dtype == torch.complex64 and r.dtype == torch.float32
    return float(torch.mean(r * r)), (torch.conj(win) * g).imag.numpy()


def max_over_rms(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.sqrt(np.mean(b * b)))


def engine_step(h, **kwargs):
    """One engine body from the phase the hologram holds, the gradient kept: (gradient, loss, phase afterwards)."""
    h.optimize("CG", maxiter=1, verbose=False, keep_gradient=True, **kwargs)
    return h.get_cg_gradient(), h.flags["loss_result"], np.array(h.phase, copy=True)


def check_step(name, h, loss_yardstick="gradient"):
    """
    Teacher-forced step of ``h`` against the restatement from the same phase and inputs: gradient (both measures), loss,
    in float64 the phase after the step; every pixel with |g| > MOVES_ABOVE moved.  Prints the engine's errors next to their
    yardsticks and returns them.
    """
    f64 = np.dtype(h.dtype) == np.float64
    phase0 = np.array(h.phase, dtype=np.float64)
    amp, kern, target = held_inputs(h)
    loss_ref, g_ref = np_loss_and_gradient(phase0, amp, kern, target)
    after_ref = adam_step(phase0, np.zeros_like(phase0), np.zeros_like(phase0), g_ref, 1)[0]
    grad, loss, after = engine_step(h)
    got = dict(l2=rel_l2(grad, g_ref), max=max_over_rms(grad, g_ref), loss=abs(loss - loss_ref) / loss_ref)
    if f64:
        yard = {}
        got["phase"] = rel_l2(after, after_ref)
        bound = dict(l2=1e-9, max=1e-9, loss=1e-12, phase=1e-9)
    else:
        loss32, g32 = f32_loss_and_gradient(phase0, amp, kern, target)
        yard = dict(l2=rel_l2(g32, g_ref), max=max_over_rms(g32, g_ref))
        yard["loss"] = abs(loss32 - loss_ref) / loss_ref if loss_yardstick == "loss" else yard["l2"]
        floor = 0.0 if is_pow2(h.shape) else 1e-5
        bound = {k: max(3 * v, floor) for k, v in yard.items()}
    print(f"cg shapes {name} {np.dtype(h.dtype).name}: engine " + " ".join(f"{k} {v:.3e}" for k, v in got.items())
          + (" | d32 " + " ".join(f"{k} {v:.3e}" for k, v in yard.items()) if yard else "")
          + " | bound " + " ".join(f"{k} {v:.3e}" for k, v in bound.items()))
    assert grad.shape == h.slm_shape and grad.dtype == h.dtype and np.all(np.isfinite(grad)) and np.isfinite(loss)
    for k, v in got.items():
        assert v <= bound[k], (name, k, v, bound[k])
    big = np.abs(g_ref) > MOVES_ABOVE                          # (holds for the tail pixels: test_residues)
    moved = after.astype(np.float64) != phase0
    assert np.all(moved[big]), (name, np.argwhere(big & ~moved)[:8])
    return got, yard


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def torch_adam_trajectory(phase, amp, kernel, target, steps, lr, betas, eps):
    """The loop as torch writes it: float64 torch.fft, autograd through the default loss, torch.optim.Adam."""
    shape = target.shape
    i0, i1, i2, i3 = toolbox.unpad(shape, phase.shape)
    p = torch.tensor(phase, dtype=torch.float64, requires_grad=True)
    a, k, t = torch.tensor(amp, dtype=torch.float64), torch.tensor(kernel, dtype=torch.float64), torch.tensor(target, dtype=torch.float64)
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    grad1, phases, losses = None, [], []
    for _ in range(steps):
        opt.zero_grad()
        n = torch.zeros(shape, dtype=torch.complex128)
        n[i0:i1, i2:i3] = a * torch.exp(1j * (p + k))
        A = torch.abs(torch.fft.fftshift(torch.fft.fft2(torch.fft.fftshift(n), norm="ortho")))
        loss = torch.nn.functional.mse_loss(A / torch.sqrt(torch.sum(A * A)), t, reduction="mean")
        loss.backward()
        grad1 = p.grad.detach().numpy().copy() if grad1 is None else grad1
        opt.step()
        losses.append(float(loss.detach()))
        phases.append(p.detach().numpy().copy())
    return grad1, phases, np.array(losses)


@pytest.mark.parametrize("hyper", HYPER, ids=("lr0.02-b0.8-0.99-eps1e-6", "lr0.1-b0-0.5-eps1e-3"))
def test_restatement_matches_torch_adam(hyper):
    """The restatement at a general-length geometry with both tails (P % 4 = S % 4 = 3) and Adam settings other than the
    defaults -- where eps enters relative to the bias corrections, beta1 = 0 -- against autograd + torch.optim.Adam in
    float64: gradient of step 1, phases after each of 5 steps, losses; relative L2 < 1e-10 as in test_cg.py."""
    shape, slm = (101, 75), (33, 51)
    i = make_inputs(shape, slm, True)
    target, amp = i["target"] / np.linalg.norm(i["target"]), i["amp"] / np.linalg.norm(i["amp"])
    ours = np_trajectory(i["phase"], amp, i["kernel"], target, 5, **hyper)
    theirs = torch_adam_trajectory(i["phase"], amp, i["kernel"], target, 5, **hyper)
    d = {"grad_1": rel_l2(ours[0], theirs[0]), "loss": rel_l2(ours[2], theirs[2])}
    d.update({f"phase_{k + 1}": rel_l2(ours[1][k], theirs[1][k]) for k in range(5)})
    print(hyper, d)
    assert np.all(np.diff(theirs[2]) != 0)                      # the phase moves: the trajectory is not a fixed point
    for name, value in d.items():
        assert value < 1e-10, (name, value)


def test_residues():
    """Every geometry of the GPU tests below keeps the element-count residues (and the transform family) it was chosen for,
    and the reference gradient of each tail pixel is large enough for the 'every pixel moved' assertion to look at it."""
    assert set(RESIDUES) == set(TAILS) | set(ROWS) | {BIG}
    for (shape, slm), want in RESIDUES.items():
        assert ((shape[0] * shape[1]) % 4, (slm[0] * slm[1]) % 4) == want, (shape, slm)
    assert [is_pow2(shape) for shape, _ in TAILS] == [True, True, True, False, False, False]
    assert sorted({r[1] for r in (RESIDUES[g] for g in TAILS)}) == [0, 1, 2, 3]
    assert sorted({r[0] for r in (RESIDUES[g] for g in TAILS)}) == [0, 1, 2, 3]
    for shape, slm in ROWS:
        assert is_pow2(shape) and shape[0] == 64 and (slm[1] == shape[1] or (slm[1] % 2 == 1 and slm[1] < shape[1] // 2))
    for shape, slm in TAILS:
        tail = (slm[0] * slm[1]) % 4
        for arrays in (True, False):
            i = make_inputs(shape, slm, arrays)
            amp = 1 / np.sqrt(slm[0] * slm[1]) if i["amp"] is None else i["amp"] / np.linalg.norm(i["amp"])
            _, g = np_loss_and_gradient(i["phase"], amp, i["kernel"], i["target"] / np.linalg.norm(i["target"]))
            assert np.mean(np.abs(g) > MOVES_ABOVE) > 0.98, (shape, slm, arrays)
            if tail:
                assert np.all(np.abs(g.ravel()[-tail:]) > MOVES_ABOVE), (shape, slm, arrays, g.ravel()[-tail:])


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _id(geometry):
    (ph, pw), (sh, sw) = geometry
    return f"{ph}x{pw}-{sh}x{sw}"


@pytest.mark.gpu
@pytest.mark.parametrize("arrays", (True, False), ids=("amp+kernel", "scalar"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("geometry", TAILS, ids=_id)
def test_tails(geometry, dtype, arrays):
    """
    One teacher-forced step at element counts that leave one, two or three pixels to the tail lane of cg_adam_kernel
    (S % 4, with the reads of amp[k] / kern[k] and the write of grad[k]) and of cg_seed_kernel (P % 4: general lengths
    only), with and without amplitude and kernel arrays.  Measured on the MI355X: DESIGN.md 6.6.
    """
    shape, slm = geometry
    check_step(f"tails {_id(geometry)} {'arrays' if arrays else 'scalar'}", hologram_of(shape, slm, arrays, dtype))


@pytest.mark.gpu
def test_tail_moments_persist():
    """(101, 75) / (33, 51), float64, five free-running steps: phases after each step and the losses <= 1e-9 against the
    restatement -- the moments m and v of the tail pixels carry over from step to step like everyone else's."""
    shape, slm = (101, 75), (33, 51)
    h = hologram_of(shape, slm, True, np.float64)
    amp, kern, target = held_inputs(h)
    _, phases, losses = np_trajectory(h.phase, amp, kern, target, 5)
    snaps = []
    h.optimize("CG", maxiter=5, verbose=False, callback=lambda hh: snaps.append(np.array(hh.phase, copy=True)) and False)
    got = {f"phase_{k + 1}": rel_l2(snaps[k], phases[k]) for k in range(5)}
    got["loss"] = rel_l2(h.stats["flags"]["loss_result"], losses)
    got["tail_5"] = rel_l2(snaps[4].ravel()[-3:], phases[4].ravel()[-3:])
    print(f"cg shapes tail trajectory f64: engine {got} | bound 1e-9")
    assert len(snaps) == 5 and h.iter == 5
    for name, value in got.items():
        assert value <= 1e-9, (name, value)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("geometry", ROWS, ids=_id)
def test_row_forms_with_nf_out(geometry, dtype):
    """
    f2n_complex at rows of 512 .. 4096 points: the straight-line form of row_kernel (1024, 2048: raw buffer stores of the
    complex nearfield, doubled byte range, negative columns wrapping out of range) and the branching one (512, 4096; the
    narrow SLM at 4096 runs its shifted eight-slot instance).  The dispatch record proves the instance ran.  Full-width
    SLMs take the scalar amplitude, the narrow ones amplitude and kernel arrays.
    """
    shape, slm = geometry
    full = slm[1] == shape[1]
    h = hologram_of(shape, slm, not full, dtype)
    check_step(f"rows {_id(geometry)}", h)
    rec = dispatch_of(h)
    r = "double" if np.dtype(dtype) == np.float64 else "float"
    ns = 8 if (shape[1] == 4096 and not full) else 16
    assert rec.count("row_kernel", flags=("nf_out",), R=r, N=shape[1], MODE=1, NS=ns) == 1, rec
    assert rec.count("row_kernel", flags=("nf_out",)) == 1 and rec.count("cg_adam_kernel", R=r) == 1, rec


@functools.lru_cache(maxsize=None)
def device_cu_count():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.gpu
def test_grid_stride_trip_and_wide_reduction():
    """
    Float32, padded 2048 x 2048, SLM 1152 x 1920, array amplitude: P / 4 lane-steps against 256 * min(ceil(P / 256), 8 n_cu)
    lanes, so every lane of cg_seed_kernel makes a second trip, and reduce_partials folds 8 n_cu partial sums.  The loss is
    the one output that sees every partial sum: within 3 * d32_loss, the float32 CPU evaluation's own loss error.
    """
    shape, slm = BIG
    P, n_cu = shape[0] * shape[1], device_cu_count()
    if not P // 4 > 256 * min(-(-P // 256), 8 * n_cu):
        pytest.skip(f"{n_cu} compute units: the seed pass covers {shape} in one trip")
    i, dt = make_inputs(shape, slm, True), np.float32
    h = Hologram(i["target"].astype(dt), amp=i["amp"].astype(dt), phase=i["phase"].astype(dt), slm_shape=slm, dtype=dt)
    check_step(f"grid-stride {_id(BIG)}", h, loss_yardstick="loss")
    rec = dispatch_of(h)
    assert rec.count("cg_seed_kernel", R="float") == 1, rec


@pytest.mark.gpu
@pytest.mark.parametrize("hyper", HYPER, ids=("lr0.02-b0.8-0.99-eps1e-6", "lr0.1-b0-0.5-eps1e-3"))
def test_adam_numerics(hyper):
    """Case A, float64, five free-running steps through optimize("CG", optimizer_kwargs=...) with Adam settings other
    than the defaults: phases after each step and losses <= 1e-9 against the restatement."""
    h = make_hologram("A", np.float64)
    amp, kern, target = held_inputs(h)
    _, phases, losses = np_trajectory(h.phase, amp, kern, target, 5, **hyper)
    snaps = []
    h.optimize("CG", maxiter=5, verbose=False, optimizer_kwargs=dict(hyper),
               callback=lambda hh: snaps.append(np.array(hh.phase, copy=True)) and False)
    got = {f"phase_{k + 1}": rel_l2(snaps[k], phases[k]) for k in range(5)}
    got["loss"] = rel_l2(h.stats["flags"]["loss_result"], losses)
    print(f"cg shapes adam {hyper}: engine {got} | bound 1e-9")
    assert rel_l2(phases[4], phases[0]) > 1e-6                # the settings matter: the phase keeps moving
    for name, value in got.items():
        assert value <= 1e-9, (name, value)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_zero_farfield_pixels(dtype):
    """
    The A > 0 guard of cg_seed_one: padded = SLM = 64 x 64, uniform amplitude 1 / 64, phase 0 -- the farfield is one pixel and
    exact zeros elsewhere (asserted on get_farfield(): otherwise this test would be vacuous).  After one step the loss is
    finite and the restatement's, the gradient and the phase are finite everywhere.  The gradient itself is not compared:
    |F| is not differentiable at 0, the guard's 0 is a convention and a reference that rounds differently has noise there.

    Loss bound, float64: relative 1e-12.  Float32: 32 roundings of 2^-24 = 1.9e-6.  Half of this loss is the one lit
    pixel's r^2, r = A / s - t: A carries at most the roundings of twelve radix-2 stages of the two transforms, then one
    each for the square root, 1 / s, the product and the difference (sixteen), and squaring doubles a relative error; the
    sum itself runs in double.
    """
    dt = np.dtype(dtype).type
    _, gold = load_golden("cg_A_f64")
    h = Hologram(gold["target"].astype(dt), phase=np.zeros((64, 64), dtype=dt), slm_shape=(64, 64), dtype=dt)
    ff = h.get_farfield()
    zeros = int(np.sum(ff == 0))
    amp, kern, target = held_inputs(h)
    loss_ref, _ = np_loss_and_gradient(np.zeros((64, 64)), amp, kern, target)
    grad, loss, after = engine_step(h)
    err = abs(loss - loss_ref) / loss_ref
    bound = 1e-12 if dt is np.float64 else 32 * 2.0 ** -24
    print(f"cg shapes zero farfield {np.dtype(dt).name}: {zeros} exact zeros of {ff.size}, loss {loss:.6e} rel err {err:.3e} | bound {bound:.1e}")
    assert zeros >= 1
    assert np.isfinite(loss) and err <= bound, (loss, loss_ref, err)
    assert np.all(np.isfinite(grad)) and np.all(np.isfinite(after))


@pytest.mark.gpu
def test_cg_after_gs_matches_restatement():
    """Case A, float64: three GS iterations, then three CG bodies -- which start from whatever the fused loop left on the
    device (the G of its last row launch, n2f's shortcut) -- within 1e-9 of the restatement started from the phase GS
    ended on."""
    h = make_hologram("A", np.float64)
    h.optimize("GS", maxiter=3, verbose=False)
    start = np.array(h.phase, copy=True)
    amp, kern, target = held_inputs(h)
    _, phases, losses = np_trajectory(start, amp, kern, target, 3)
    h.optimize("CG", maxiter=3, verbose=False)
    got = dict(phase=rel_l2(h.phase, phases[2]), loss=rel_l2(h.stats["flags"]["loss_result"][-3:], losses))
    print(f"cg shapes after GS f64: engine {got} | bound 1e-9")
    assert h.iter == 6 and rel_l2(phases[2], start) > 1e-3
    for name, value in got.items():
        assert value <= 1e-9, (name, value)


@pytest.mark.gpu
def test_reset_restarts_adam():
    """hgs_reset between two hgs_cg_iterate calls: the next body, restart = 0, is Adam's first -- its step is
    -lr g / (|g| + eps) of the gradient at the phase it starts from (test_restart_and_chunking's assertion, reached
    through cg_t = 0 in hgs_reset instead of the restart flag), and that gradient is the restatement's."""
    h = make_hologram("A", np.float64)
    e = h._get_engine()
    e.cg_iterate(3, lr=LR, restart=True)
    before = e.get(L.PHASE)[0]
    e.reset()
    e.cg_iterate(1, lr=LR, restart=False, keep_grad=True)
    after, g = e.get(L.PHASE)[0], e.get_cg_grad()
    amp, kern, target = held_inputs(h)
    _, g_ref = np_loss_and_gradient(before, amp, kern, target)
    big = np.abs(g) > 10 * EPS
    assert big.sum() > 50 and rel_l2(g, g_ref) <= 1e-9
    np.testing.assert_allclose((after - before)[big], (-LR * g / (np.abs(g) + EPS))[big], rtol=1e-6, atol=0)
    assert np.all(np.abs(after - before)[big] > 0.9 * LR)


@pytest.mark.gpu
def test_loss_buffer_regrow_and_zero_bodies():
    """The per-body loss buffer grows between calls (2 bodies, then 5: synchronise, free, allocate): losses and final
    phase of the second call are those of a fresh engine's five bodies bit for bit.  Zero bodies: an empty array, the
    phase untouched."""
    h, fresh = make_hologram("A", np.float32), make_hologram("A", np.float32)
    e, f = h._get_engine(), fresh._get_engine()
    start = e.get(L.PHASE)[0]
    none = e.cg_iterate(0, lr=LR)
    assert none.shape == (0,) and none.dtype == np.float64
    np.testing.assert_array_equal(e.get(L.PHASE)[0], start)
    assert len(e.cg_iterate(2, lr=LR)) == 2
    assert np.any(e.get(L.PHASE)[0] != start)
    e.set(L.PHASE, start)
    loss, want = e.cg_iterate(5, lr=LR, restart=True), f.cg_iterate(5, lr=LR)
    assert loss.shape == (5,) and np.all(np.isfinite(loss)) and np.all(np.diff(loss) != 0)
    np.testing.assert_array_equal(loss, want)
    np.testing.assert_array_equal(e.get(L.PHASE)[0], f.get(L.PHASE)[0])
    none = e.cg_iterate(0, lr=LR)
    assert none.shape == (0,)
    np.testing.assert_array_equal(e.get(L.PHASE)[0], f.get(L.PHASE)[0])
