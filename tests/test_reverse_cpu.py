"""The chunked backward sweep of pde_opt_amd.reverse on CPU tensors, with a toy linear step and no engine: which state
starts a chunk, where the forward pass stops and when a save point's cotangent is added, against a numpy loop that holds
every state and knows no chunks.

The toy problem.  The state is ``(B, n)`` in fp64.  Substep ``i`` multiplies it by ``d_i``, one factor per cell that
depends on the step size (so the clipped last step matters); the adjoint substep adds ``sum(lam * u_i)`` over the cells
into a per-environment fp64 block and multiplies ``lam`` by ``d_i``.

The bound of the comparison with numpy.  Both sides evaluate the same sums of products in fp64, possibly in another
order (torch and numpy sum the cells of a row as they like), so each lies within ``gamma_m S`` of the exact value and
they differ by at most ``2 gamma_m S``: ``gamma_m = m u / (1 - m u)`` with ``u = 2^-53`` (Higham, Accuracy and Stability
of Numerical Algorithms, Lemma 3.1), ``m`` the largest number of roundings on the way from the inputs to one output,
and ``S`` the same expression evaluated with absolute values in place of every input.  On the way to an entry of ``lam0``
lie at most ``N`` factors ``d_i`` and ``N + 1`` additions of cotangents (``2 N + 1``), the split of a cotangent
(``1 - theta`` and one product: 2), and, where the cotangent is a residual of the states, the ``N`` products behind a
state, its interpolation (3) and the subtraction (1).  An entry of the gradient block adds the ``N`` products behind
``u_i``, the product ``lam * u_i``, ``n - 1`` additions over the cells and ``N`` over the substeps.  In all
``m <= 5 N + n + 7``, which is 47 for ``N = 7`` and ``n = 5``: ``2 gamma_m = 1.05e-14``."""
import math

import numpy as np
import pytest
import torch

from pde_opt_amd import reverse

B, CELLS, DT0 = 2, 5, 1.0
# N = 7 substeps, the last clipped to 0.5: saves at ts[0], on a step edge (2), twice inside substep 4 (theta 0.3 and 0.8)
# and at the end
TS = np.array([0.0, 2.0, 3.3, 3.8, 6.5])
N = 7
RNG = np.random.default_rng(11)
A = RNG.uniform(-0.3, 0.3, (N, CELLS))
Y0 = RNG.standard_normal((B, CELLS))
COTS = RNG.standard_normal((len(TS), B, CELLS))     # the cotangents known beforehand
TARGETS = RNG.standard_normal((len(TS), B, CELLS))  # the data of the residual form
BOUND = 2.0 * (47 * 2.0**-53) / (1.0 - 47 * 2.0**-53)


def _factors(steps):
    return [1.0 + (dt / DT0) * A[i] for i, dt in enumerate(steps)]


def _reference(ts, y0, cot_of_save, first_too):
    """``(grad (B,), lam0, S_grad, S_lam0)`` from every state held at once: ``cot_of_save(q, pred, pred_abs)`` is the
    cotangent of save q and its magnitude; ``first_too`` adds the cotangent of the initial state as well.  The ``S`` are
    the same sums with absolute values throughout."""
    steps, _ = reverse.schedule(ts, DT0)  # the step sizes alone: where the saves fall is found below
    n, d = len(steps), _factors(steps)
    y, ya = [y0], [np.abs(y0)]
    for i in range(n):
        y.append(y[i] * d[i])
        ya.append(ya[i] * np.abs(d[i]))
    g = [np.zeros_like(y0) for _ in range(n + 1)]
    ga = [np.zeros_like(y0) for _ in range(n + 1)]
    for q, tq in enumerate(ts):
        pos = (tq - ts[0]) / DT0
        i = min(n, int(math.ceil(pos - 1e-9)))
        on_edge = i == 0 or abs(min(ts[0] + i * DT0, ts[-1]) - tq) < 1e-12
        if on_edge:
            c, ca = cot_of_save(q, y[i], ya[i])
            g[i], ga[i] = g[i] + c, ga[i] + ca
        else:
            a, b = ts[0] + (i - 1) * DT0, min(ts[0] + i * DT0, ts[-1])
            theta = (tq - a) / (b - a)
            c, ca = cot_of_save(q, y[i - 1] + theta * (y[i] - y[i - 1]), ya[i - 1] + theta * (ya[i] + ya[i - 1]))
            g[i - 1], ga[i - 1] = g[i - 1] + (1.0 - theta) * c, ga[i - 1] + (1.0 - theta) * ca
            g[i], ga[i] = g[i] + theta * c, ga[i] + theta * ca
    lam, lama = g[n], ga[n]
    if n == 0 and not first_too:
        lam, lama = np.zeros_like(y0), np.zeros_like(y0)
    grad, grada = np.zeros(y0.shape[0]), np.zeros(y0.shape[0])
    for s in range(n - 1, -1, -1):
        grad, grada = grad + np.sum(lam * y[s], axis=1), grada + np.sum(lama * ya[s], axis=1)
        lam, lama = lam * d[s], lama * np.abs(d[s])
        if s > 0 or first_too:
            lam, lama = lam + g[s], lama + ga[s]
    return grad, lam, grada, lama


def _toy(ts):
    steps, saves = reverse.schedule(ts, DT0)
    d = [torch.as_tensor(f) for f in _factors(steps)]
    Y = torch.as_tensor(Y0.copy())

    def step(i):
        Y.mul_(d[i])

    def adjoint(s, u, lam, grad, second=None):
        for block in (grad, second):
            if block is not None:
                block += (lam * u).sum(dim=1)
        lam.mul_(d[s])

    return Y, len(steps), saves, step, adjoint


def _known(ts, chunk, tails=((),)):
    """the form of the GPE gradients: cotangents known beforehand, the one of the initial state included"""
    Y, n, saves, step, adjoint = _toy(ts)
    blocks, lam0, chunks = reverse.known_cotangent_sweep(Y, n, chunk, saves, COTS[:len(ts)], list(tails), step, adjoint)
    return [None if g is None else g.numpy() for g in blocks], lam0.numpy(), chunks


def _residual(ts, chunk):
    """the form of fieldmu: the cotangents are residuals of the states the forward pass visits; the cotangent of the
    initial state has no use and is left out"""
    Y, n, saves, step, adjoint = _toy(ts)
    need_prev = {i - 1 for i, theta in saves if theta is not None}
    cot, prev = {}, None

    def visit(i):
        nonlocal prev
        for q, (k, theta) in enumerate(saves):
            if k == i:
                pred = Y if theta is None else prev + theta * (Y - prev)
                reverse.add_save_cotangent(cot, i, theta, pred - torch.as_tensor(TARGETS[q]))
        if i in need_prev:
            prev = Y.clone()

    grad = torch.zeros(B, dtype=torch.float64)
    starts = reverse.forward_pass(Y, n, chunk, step, visit=visit)
    chunks = len(starts)
    lam0 = reverse.backward_pass(Y, starts, n, chunk, step, lambda s, u, lam: adjoint(s, u, lam, grad),
                                 lambda s: cot.get(s) if s > 0 else None)
    return [grad.numpy()], lam0.numpy(), chunks


def test_the_schedule_of_the_toy_problem_has_the_saves_the_test_is_about():
    steps, saves = reverse.schedule(TS, DT0)
    assert steps == [1.0] * 6 + [0.5] and len(steps) == N
    assert saves[0] == (0, None) and saves[1] == (2, None) and saves[4] == (7, None)
    assert [i for i, _ in saves[2:4]] == [4, 4]
    for (_, theta), want in zip(saves[2:4], (0.3, 0.8)):
        assert abs(theta - want) < 1e-12


@pytest.mark.parametrize("form", ["known", "residual"])
def test_chunking_leaves_the_bits_alone_and_the_sweep_equals_the_loop_that_holds_every_state(form):
    run = _known if form == "known" else _residual
    if form == "known":
        want = _reference(TS, Y0, lambda q, pred, pred_abs: (COTS[q], np.abs(COTS[q])), first_too=True)
    else:
        want = _reference(TS, Y0, lambda q, pred, pred_abs: (pred - TARGETS[q], pred_abs + np.abs(TARGETS[q])), first_too=False)
    grad_ref, lam_ref, grad_scale, lam_scale = want
    first = None
    for chunk in (1, 3, N, N + 3):
        (grad,), lam0, chunks = run(TS, chunk)
        assert chunks == math.ceil(N / chunk)
        if first is None:
            first = grad, lam0
        assert grad.tobytes() == first[0].tobytes() and lam0.tobytes() == first[1].tobytes(), chunk
    grad, lam0 = first
    print(form, "grad", np.max(np.abs(grad - grad_ref) / grad_scale), "lam0", np.max(np.abs(lam0 - lam_ref) / lam_scale), "bound", BOUND)
    assert np.all(np.abs(grad - grad_ref) <= BOUND * grad_scale)
    assert np.all(np.abs(lam0 - lam_ref) <= BOUND * lam_scale)
    assert np.max(np.abs(grad_ref)) > 0.1 and np.max(np.abs(lam_ref)) > 0.1  # the comparison is not one of zeros


def test_a_solve_without_a_substep_returns_the_cotangent_and_a_zero_gradient():
    (grad,), lam0, chunks = _known(TS[:1], 1)
    assert lam0.tobytes() == COTS[0].tobytes() and not grad.any() and chunks == 1
    (grad,), lam0, chunks = _residual(TS[:1], 1)
    assert not lam0.any() and not grad.any() and chunks == 0


@pytest.mark.parametrize("chunk", [1, 3, N])
def test_a_second_gradient_block_present_or_absent(chunk):
    (one,), lam_one, _ = _known(TS, chunk)
    (first, second), lam0, _ = _known(TS, chunk, tails=((), None))
    assert second is None and first.tobytes() == one.tobytes() and lam0.tobytes() == lam_one.tobytes()
    (first, second), lam0, _ = _known(TS, chunk, tails=((), ()))
    assert first.tobytes() == one.tobytes() and second.tobytes() == one.tobytes() and lam0.tobytes() == lam_one.tobytes()


def test_the_sweep_leaves_the_callers_cotangents_alone():
    before = COTS.copy()
    _known(TS, 3)
    assert COTS.tobytes() == before.tobytes()
